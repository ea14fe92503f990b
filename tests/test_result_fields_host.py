"""The table of the optional result fields (``io.OPTIONAL_FIELDS``) against the ``StacData`` dataclass, and a result with all of them
through two shard files and a manifest.  Four frames, three keypoints; no device is touched."""

import dataclasses

import numpy as np

import host_scaffold as hs


def _result(rng, T=4, K=3, nq=5, nb=2):
    from stac_mjx_amd import io

    f32 = lambda *shape: rng.random(shape, dtype=np.float32)  # noqa: E731
    u8 = lambda: rng.integers(0, 2, (T, K)).astype(np.uint8)  # noqa: E731
    return io.StacData(qpos=f32(T, nq), xpos=f32(T, nb, 3), xquat=f32(T, nb, 4), marker_sites=f32(T, K, 3), offsets=f32(K, 3),
                       kp_data=f32(T, 3 * K), names_qpos=[f"q{i}" for i in range(nq)], names_xpos=[f"b{i}" for i in range(nb)],
                       kp_names=[f"k{i}" for i in range(K)], qvel=f32(T, nq - 1), kp_gap=rng.integers(1, 9, (T, K)).astype(np.int32),
                       qpos_raw=f32(T, nq), kp_rejected_pairwise=u8(), kp_swapped=u8(), kp_rejected=u8())


def test_table_against_dataclass():
    from stac_mjx_amd import io

    fields = {f.name: f for f in dataclasses.fields(io.StacData)}
    names = [name for name, _ in io.OPTIONAL_FIELDS]
    assert names == ["kp_gap", "kp_rejected", "qpos_raw", "kp_rejected_pairwise", "kp_swapped"]  # the order of the datasets in a file
    assert list(fields)[-1] == "kp_rejected"  # (positional construction: it stays the trailing field)
    plain = io.StacData(*[np.zeros((1, 1), np.float32)] * 6, ["q"], ["b"], ["k"])
    for name, dtype in io.OPTIONAL_FIELDS:
        assert name in fields and fields[name].default_factory is not dataclasses.MISSING
        empty = fields[name].default_factory()
        assert isinstance(empty, np.ndarray) and empty.size == 0
        assert getattr(plain, name).size == 0 and name not in plain.as_dict()
        assert dtype in (None, np.uint8)
    full = _result(np.random.default_rng(0))
    assert [k for k in full.as_dict() if k in names] == [f for f in fields if f in names]  # all five, once non-empty
    for name in names:  # ... and each on its own
        one = dataclasses.replace(plain, **{name: getattr(full, name)})
        assert [k for k in one.as_dict() if k in names] == [name]


def test_all_fields_through_shards(tmp_path, rodent_cfg):
    from stac_mjx_amd import io

    cfg, whole = hs.stage_cfg(rodent_cfg), _result(np.random.default_rng(1))
    names = [name for name, _ in io.OPTIONAL_FIELDS]
    per_frame = [f.name for f in dataclasses.fields(io.StacData) if f.name not in ("offsets", "names_qpos", "names_xpos", "kp_names")]
    assert set(names) < set(per_frame)
    for suffix in [".npz"] + ([".h5"] if io.h5py is not None else []):
        d = tmp_path / suffix[1:]
        d.mkdir()
        one = io.load_stac_result(io.save_data_to_h5(config=cfg, file_path=d / f"whole{suffix}", **whole.as_dict()))[1]
        ik = d / f"ik{suffix}"
        for r, rows in enumerate((slice(0, 2), slice(2, 4))):  # two clips of two frames, one per rank
            part = dataclasses.replace(whole, **{name: getattr(whole, name)[rows] for name in per_frame})
            io.save_data_to_h5(config=cfg, file_path=io.shard_path(ik, r, 2), **part.as_dict())
        manifest = io.write_manifest(io.manifest_path(ik), ik, 2, 2, 2)
        back = io.load_stac_result(manifest)[1]
        for f in dataclasses.fields(io.StacData):
            a, b, w = getattr(back, f.name), getattr(one, f.name), getattr(whole, f.name)
            if isinstance(w, list):
                assert a == b == w, f.name
                continue
            assert a.dtype == b.dtype == w.dtype and a.shape == w.shape and a.size, f.name
            np.testing.assert_array_equal(a, b, err_msg=f.name)
            np.testing.assert_array_equal(a, w, err_msg=f.name)
        if suffix == ".npz":  # the datasets of a file: the reference's, then the optional ones in the table's order
            with np.load(io.resolve_output_path(io.shard_path(ik, 0, 2))) as f:
                assert [k for k in f.files if k in names] == names
