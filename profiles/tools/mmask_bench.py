"""The offset phase on observed keypoints only (stac.offset_mask: ``stac_mmask_partial`` + ``stac_mmask_finish``) on one GPU, beside
the ``stac_fk`` call that feeds it and the unmasked phase it stands in for, ``stac_m_phase_partial`` + ``stac_m_phase_finish``, on the
same inputs (DESIGN.md "Offsets from observed keypoints", profiles/mmask/mmask_bench.json).

  python profiles/tools/mmask_bench.py --out profiles/mmask/mmask_bench.json [--frames 1000,100000] [--reps 20]

The model is the golden rodent (K = 23, 67 bodies), the poses are seeded noise around its rest pose, 30 % of the keypoint values are
masked.  Device events around whole calls of the ``Engine`` methods, medians of ``--reps`` calls after 3 warm-up calls.  The unmasked
partial runs the kinematics itself, so the like-for-like figure is (fk + masked) over unmasked.  There is no gate: the phase is a
fraction of a percent of a fit and both reductions keep the serial order of their sums on purpose.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(Path(__file__).resolve().parent)]

from select_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", default="1000,100000")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()

    from stac_mjx_amd.engine import Engine
    from stac_mjx_amd.fit_model import finish_fit_setup
    from stac_mjx_amd.mjcf import ModelTables

    if not torch.cuda.is_available():
        raise SystemExit("mmask_bench needs a GPU: nothing is measured without one")
    golden = ROOT / "tests" / "golden"
    cfg = json.loads((golden / "rodent_model_cfg.json").read_text())
    fs = finish_fit_setup(ModelTables.load(golden / "rodent_tables.npz"), cfg, list(cfg["KEYPOINT_MODEL_PAIRS"].keys()))
    eng = Engine(fs.tables, fs.lb, fs.ub)
    K, lam = eng.K, float(cfg["M_REG_COEF"])
    m0 = eng.get_site_pos()
    dreg = torch.as_tensor(np.asarray(fs.is_regularized, np.float32)).cuda()
    result = {"tool": "profiles/tools/mmask_bench.py", "command": "python " + " ".join(sys.argv), "device": torch.cuda.get_device_name(0),
              "n_kp": K, "nbody": eng.nbody, "masked_share": 0.3,
              "timing": f"device events around whole calls, medians of {args.reps} calls after 3 warm-up calls", "cases": []}
    for T in (int(v) for v in args.frames.split(",")):
        rng = np.random.default_rng(7)
        q = np.tile(fs.tables.qpos0, (T, 1)).astype(np.float32)
        q[:, 3:7] += rng.normal(0, 0.3, (T, 4)).astype(np.float32)
        q[:, 7:] += rng.normal(0, 0.2, (T, q.shape[1] - 7)).astype(np.float32)
        q = torch.as_tensor(q).cuda()
        fk = eng.fk(q, want=("xpos", "xquat", "site_xpos"))
        kp = (fk["site_xpos"] + 0.003 * torch.randn(T, K, 3, device="cuda")).reshape(T, 3 * K).contiguous()
        valid = (torch.rand(T, K, device="cuda") >= 0.3).to(torch.uint8)
        xpos, xquat = fk["xpos"], fk["xquat"]
        t_fk = timed(lambda: eng.fk(q, want=("xpos", "xquat")), args.reps, warm=3)
        t_masked = timed(lambda: eng.m_finish_masked(eng.m_partial_masked(kp, xpos, xquat, valid), m0, dreg, lam), args.reps, warm=3)
        t_plain = timed(lambda: eng.m_finish(eng.m_partial(kp, q), m0, dreg, lam), args.reps, warm=3)
        # every entry observed: the masked path gives the unmasked offsets
        ones = torch.ones_like(valid)
        same = bool(torch.equal(eng.m_finish_masked(eng.m_partial_masked(kp, xpos, xquat, ones), m0, dreg, lam)[0], eng.m_finish(eng.m_partial(kp, q), m0, dreg, lam)[0]))
        entry = {"n_frames": T, "stac_fk": t_fk, "masked_partial_and_finish": t_masked, "unmasked_partial_and_finish_with_its_own_fk": t_plain,
                 "fk_plus_masked_over_unmasked": (t_fk["ms_median"] + t_masked["ms_median"]) / t_plain["ms_median"],
                 "all_valid_offsets_equal_the_unmasked_bits": same}
        result["cases"].append(entry)
        print(json.dumps({"T": T, "fk_ms": t_fk["ms_median"], "masked_ms": t_masked["ms_median"], "unmasked_ms": t_plain["ms_median"],
                          "ratio": entry["fk_plus_masked_over_unmasked"], "all_valid_same_bits": same}), flush=True)
    if args.out:
        path = Path(args.out)
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(result, indent=1) + "\n")
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
