"""The render kernel (csrc/stac_render.hip) on the scenes of tests/test_render_rule_host.py, through stac_render_scene_create
/ stac_render on sentinel-filled outputs: bit for bit against the float build of tests/tools/render_ref.c (the tolerance-0
contract, here also for cameras inside solids, views along an axis and ties), and against tests/render_rule.py, the frame
rule stated from solid membership in float64 on the host, with the bounds of the float build there: seg and hit / no-hit
equal, rgb within one step, depth within 1e-5 relative, on the pixels that neither the double build's ``amb`` nor the
rule's ``edge`` marks, which are at most AMB_CAP of an image.  Each single-primitive scene renders its 8 poses as the frames
of one launch."""

import numpy as np
import pytest

from render_cases import (CAPSULE_INSIDE_VIEWS, INSIDE_KINDS, OUTSIDE_KINDS, RULE_NBODY, RULE_SIZES, TIE_CLEAR, TIE_OPAQUE,
                          RenderRef, assert_same, compare_with_rule, eroded, gpu_render, random_scene, rodent_render_args, rodent_scene,
                          rule_cases, rule_picture)

pytestmark = pytest.mark.gpu

CASES = rule_cases()


@pytest.fixture(scope="module")
def refs():
    return RenderRef("float"), RenderRef("double")


@pytest.fixture(scope="module")
def eng(rodent_setup_legacy):
    from stac_mjx_amd.engine import Engine

    fs = rodent_setup_legacy
    e = Engine(fs.tables, fs.lb, fs.ub, device="cuda:0")
    assert e.nbody == RULE_NBODY
    return e


def hold_kernel(refs, eng, name, args, W, H, single=False):
    """One launch over the scene's frames; returns (kernel picture, float build's picture, rule picture)."""
    from stac_mjx_amd.render import RenderSceneHandle

    t, nbody, xpos, xquat, kp, markers, show, cams, tanh = args
    h = RenderSceneHandle(eng, t)
    got = gpu_render(h, xpos, xquat, kp, markers, show, cams, tanh, W, H)
    h.close()
    want = refs[0].render(*args, W, H)
    assert_same(got, want[:3], f"{name} {W}x{H}")
    amb = refs[1].render(*args, W, H)[3]
    rel, share = compare_with_rule(got, rule_picture(name, args, W, H), amb, single, 1e-5, f"{name} {W}x{H} kernel")
    print(f"{name} {W}x{H}: kernel depth against the rule {rel:.3e}, excluded share {share:.4f}")
    return got, want, rule_picture(name, args, W, H)


@pytest.mark.parametrize("W,H", RULE_SIZES)
@pytest.mark.parametrize("kind", OUTSIDE_KINDS)
def test_every_type_from_outside(refs, eng, kind, W, H):
    got, _, rule = hold_kernel(refs, eng, f"outside_{kind}", CASES[f"outside_{kind}"].args, W, H, single=True)
    if kind in ("capsule", "cylinder") and W % 2 and H % 2:  # the centre pixel looks exactly along the axis
        assert got[1][7, H // 2, W // 2] == 7


@pytest.mark.parametrize("W,H", RULE_SIZES)
@pytest.mark.parametrize("transparent", [False, True])
@pytest.mark.parametrize("kind", INSIDE_KINDS)
def test_every_type_from_inside(refs, eng, kind, transparent, W, H):
    c = CASES[f"inside_{kind}_{'transparent' if transparent else 'opaque'}"]
    got, _, _ = hold_kernel(refs, eng, c.name, c.args, W, H)
    for f, solid in enumerate(c.hidden):
        assert not (got[1][f] == solid).any() and (got[1][f] == 1).sum() >= 100


@pytest.mark.parametrize("W,H", RULE_SIZES)
def test_camera_inside_a_capsule_does_not_see_it(refs, eng, W, H):
    """The statement of the host test of this name, of the kernel's pictures."""
    from stac_mjx_amd.render import RenderSceneHandle

    pics = []
    for name in ("inside_capsule_opaque", "inside_capsule_transparent"):
        t, nbody, xpos, xquat, kp, markers, show, cams, tanh = CASES[name].args
        h = RenderSceneHandle(eng, t)
        pics.append(gpu_render(h, xpos, xquat, kp, markers, show, cams, tanh, W, H))
        h.close()
    po, pc = pics
    for f, view in CAPSULE_INSIDE_VIEWS.items():
        assert not (po[1][f] == 0).any(), f"frame {f} ({view}): the capsule is seen from inside"
        assert (po[1][f] == 1).sum() >= 100, f"frame {f} ({view}): the sphere behind the capsule is not seen"
        np.testing.assert_array_equal(pc[0][f], po[0][f], err_msg=f"frame {f} ({view}): a see-through capsule tints the picture")
        np.testing.assert_array_equal(pc[1][f], po[1][f])


@pytest.mark.parametrize("W,H", RULE_SIZES)
@pytest.mark.parametrize("name", ["beyond_end", "transparency", "error_segments", "lights_none", "lights_two"])
def test_constructed_scenes(refs, eng, name, W, H):
    got, _, rule = hold_kernel(refs, eng, name, CASES[name].args, W, H)
    if name == "beyond_end":
        for f in range(4):
            assert got[1][f, H // 2, W // 2] == f % 2
    if name == "transparency":  # the tied pairs are flagged all over: their pixels are held to the rule here
        import render_rule

        T = render_rule.hit_table(*CASES[name].args, W, H)
        for lo, hi in (TIE_CLEAR, TIE_OPAQUE):
            m = eroded(np.isfinite(T[..., lo]))
            assert m.sum() >= 3
            np.testing.assert_array_equal(got[1][0][m], rule[1][0][m])
            assert np.abs(got[0][0][m].astype(int) - rule[0][0][m].astype(int)).max() <= 1
        assert (got[1][0][m] == TIE_OPAQUE[0]).all()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_scenes(refs, eng, seed):
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, 67, 23)
    hold_kernel(refs, eng, f"random{seed}", (t, 67, xpos, xquat, kp, markers, True, cams, tanh), 160, 120)


def test_rodent_through_egocentric(refs, eng, reference_dir, rodent_cfg):
    """Three stored frames through the camera on the skull, which sits among capsules and ellipsoids."""
    args = rodent_render_args(rodent_scene(reference_dir, rodent_cfg), rodent_cfg, 5, W=160, H=100)
    got, _, _ = hold_kernel(refs, eng, "rodent_camera5", args[:9], 160, 100)
    assert (got[1] >= 0).mean() > 0.05
