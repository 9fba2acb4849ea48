"""csrc/scene.hip against tests/scene_ref.py: the rendered images on decided pixels, the pixel convention against
ColChecker, batch independence, the pose and distance kernels, and the refusals.

The image bar, 1e-4 m: on a decided ray the discriminant is bounded away from zero; b^2 and c are at most dmax^2 =
25, so the fp32 discriminant error is about 1e-5 and the root error that divided by 2 sqrt(disc)."""
import numpy as np
import pytest

import scene_ref as R
from sdf_nmpc_amd import _lib
from sdf_nmpc_amd.config import Config
from sdf_nmpc_amd.scene import Scene

pytestmark = pytest.mark.gpu

IMG_ATOL = 1e-4  # metres
P, RM = R.camera_poses()
B = len(P)


def _cfg(sensor="pinhole", is_depth=False, **over):
    s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
    return Config(sensor__hfov=s["hfov"], sensor__vfov=s["vfov"], sensor__dmax=s["dmax"], sensor__is_depth=is_depth,
                  sensor__is_spherical=sensor == "spherical", **over)


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    return Scene(gpu_ctx, R.SCENE)


@pytest.fixture(scope="module")
def ref():
    """Reference values in metres and decided masks, once per (sensor, shape, is_depth)."""
    cache = {}

    def get(sensor, shape, is_depth):
        key = (sensor, tuple(shape), bool(is_depth))
        if key not in cache:
            s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
            kw = dict(is_depth=is_depth, is_spherical=sensor == "spherical")
            v = R.values(R.SCENE, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            ok = R.decided(R.SCENE, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], **kw)
            v.setflags(write=False)
            ok.setflags(write=False)
            cache[key] = (v, ok)
        return cache[key]

    return get


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_render_matches_reference_on_decided_pixels(scene, ref, sensor, shape):
    """Range and depth, normalised and raw (mm_resolution = 250: four units per metre), B = 3."""
    for is_depth in (False, True):
        cfg = _cfg(sensor, is_depth, sensor__mm_resolution=250)
        want, ok = ref(sensor, shape, is_depth)
        assert ok.mean() >= 0.98
        for normalized, per_metre in ((True, 1.0 / 5.0), (False, 4.0)):
            img = scene.render(P, RM, cfg, shape, normalized=normalized).numpy()
            assert img.shape == (B,) + tuple(shape) and img.dtype == np.float32
            gap = np.abs(img.astype(np.float64) / per_metre - want)
            print(f"\n{sensor} {shape} depth={is_depth} normalized={normalized}: worst gap on decided pixels "
                  f"{gap[ok].max():.3e} m, on all pixels {gap.max():.3e} m")
            assert gap[ok].max() <= IMG_ATOL
            assert img.max() <= np.float32(5.0 * per_metre) and (img == np.float32(5.0) * np.float32(per_metre)).any()


def test_pixel_convention_is_colcheck(scene, ref, gpu_ctx):
    """Round trip through ColChecker on the normalised range image: on the centre ray of every decided hit pixel the
    point at 0.9 t is free and the point at 1.1 t collides (when below dmax); on a miss pixel 0.9 dmax is free."""
    from sdf_nmpc_amd.collision_checker import ColChecker
    shape, s = (27, 48), R.SENSOR
    cfg = _cfg("pinhole", False)
    want, ok = ref("pinhole", shape, False)
    img = scene.render(P, RM, cfg, shape).numpy()
    dc = R.ray_dirs(*shape, s["hfov"], s["vfov"])
    hit = ok & (want < s["dmax"])
    miss = ok & (want == s["dmax"])
    assert hit.sum() > 500 and miss.sum() > 100
    cc = ColChecker(s["dmax"], s["hfov"], s["vfov"], 0.0, is_depth=False, is_spherical=False, outside="col", device=gpu_ctx)
    near = np.where(hit, 0.9 * want, 0.9 * s["dmax"])[..., None] * dc          # [B, h, w, 3], default ordering
    lab = cc.check_image_points(img, near.reshape(-1, 3)).cpu().numpy().reshape(want.shape)
    assert not lab[hit].any() and not lab[miss].any()
    far = (1.1 * want)[..., None] * dc
    lab = cc.check_image_points(img, far.reshape(-1, 3)).cpu().numpy().reshape(want.shape)
    sel = hit & (1.1 * want < s["dmax"])
    assert sel.sum() > 500 and lab[sel].all()


def test_camera_inside_a_primitive_sees_zero(scene):
    cfg = _cfg()
    p = np.array([[2.5, -0.8, 0.3], [3.0, 0.3, 0.0], [3.8, 1.0, 0.0]])  # in the sphere, the cylinder, the box
    img = scene.render(p, RM, cfg, (18, 32), normalized=False).numpy()
    assert not img.any()


def test_two_scenes_and_permutation_are_bitwise(gpu_ctx, scene):
    cfg = _cfg("pinhole", True)
    other = [Scene.sphere((2.0, 0.2, 0.0), 0.6), Scene.box((-10, -10, -1.6), (10, 10, -1.5))]
    both = Scene(gpu_ctx, [R.SCENE, other], scene_of=[1, 0, 1])
    img = both.render(P, RM, cfg, (27, 48)).numpy()
    own = [scene.render(P, RM, cfg, (27, 48)).numpy(), Scene(gpu_ctx, other).render(P, RM, cfg, (27, 48)).numpy()]
    for b, s in enumerate([1, 0, 1]):
        np.testing.assert_array_equal(img[b], own[s][b])
    assert np.abs(own[0] - own[1]).max() > 0.1
    perm = [2, 0, 1]
    np.testing.assert_array_equal(scene.render(P[perm], RM[perm], cfg, (27, 48)).numpy(), own[0][perm])
    # an instance's image does not depend on the batch around it
    np.testing.assert_array_equal(scene.render(P[1:2], RM[1:2], cfg, (27, 48)).numpy()[0], own[0][1])
    with pytest.raises(ValueError):
        Scene(gpu_ctx, [R.SCENE, other], scene_of=[0, 2, 1])
    with pytest.raises(ValueError):
        both.render(P[:2], RM[:2], cfg, (27, 48))


def test_pose_matches_numpy(scene):
    """Unnormalised quaternions, B = 70 (two blocks): 1e-15 on entries of magnitude about 1."""
    cfg = Config()
    rng = np.random.default_rng(3)
    n = 70
    x = np.zeros((n, 10))
    x[:, :3] = rng.uniform(-1, 1, (n, 3))
    x[:, 3:7] = rng.normal(0, 1, (n, 4)) * rng.uniform(0.3, 3.0, (n, 1))
    x[:, 7:] = rng.normal(0, 1, (n, 3))
    got = {k: v.numpy() for k, v in scene.pose(x, cfg).items()}
    Rb = np.stack([R.quat2rot(q) for q in x[:, 3:7]])
    B_p_C, B_R_C = np.asarray(cfg.sensor.B_p_C, float).ravel(), np.asarray(cfg.sensor.B_R_C, float)
    np.testing.assert_array_equal(got["W_p_Bo"], x[:, :3])
    for k, want in (("W_R_Bo", Rb.reshape(n, 9)), ("W_p_C", Rb @ B_p_C + x[:, :3]), ("W_R_C", (Rb @ B_R_C).reshape(n, 9))):
        err = np.abs(got[k] - want).max()
        print(f"\n{k}: max error {err:.2e}")
        assert err <= 1e-15, k
    # render_from_state is pose + render
    cfg2 = _cfg()
    a = scene.render_from_state(x[:3], cfg2, (18, 32))
    ps = scene.pose(x[:3], cfg2)
    np.testing.assert_array_equal(a.numpy(), scene.render(ps["W_p_C"], ps["W_R_C"], cfg2, (18, 32)).numpy())
    np.testing.assert_array_equal(a.pose["W_R_Bo"].numpy(), ps["W_R_Bo"].numpy())


def test_distance_matches_reference(gpu_ctx, scene):
    rng = np.random.default_rng(4)
    pts = rng.uniform([-1, -3, -2.5], [6, 3, 2.5], (700, 3))  # three blocks; inside and outside every primitive
    want = R.distance(R.SCENE, pts)
    assert (want < 0).sum() > 20 and (want > 0).sum() > 300
    got = scene.distance(pts)
    assert np.abs(got - want).max() <= 1e-12
    # two scenes: p_to_scene, and the default ordering (first half scene 0, second half scene 1)
    other = [Scene.cylinder((1.0, 1.0), 0.5, -1.0, 2.0)]
    both = Scene(gpu_ctx, [R.SCENE, other])
    p2s = rng.integers(0, 2, 700)
    w1 = R.distance(other, pts)
    assert np.abs(both.distance(pts, p2s) - np.where(p2s == 1, w1, want)).max() <= 1e-12
    assert np.abs(both.distance(pts) - np.where(np.arange(700) >= 350, w1, want)).max() <= 1e-12
    with pytest.raises(_lib.SdfnmpcError):
        both.distance(pts[:699])


def test_refusals_leave_the_output_untouched(gpu_ctx, scene):
    """SDFNMPC_E_ARG with nothing launched: the image keeps the value it was filled with."""
    h, w = 18, 32
    fill = np.full((B, h, w), -7.0, np.float32)
    out = _lib.DeviceArray.from_numpy(gpu_ctx, fill)
    dp = _lib.DeviceArray.from_numpy(gpu_ctx, P)
    dR = _lib.DeviceArray.from_numpy(gpu_ctx, RM.reshape(B, 9))
    good = dict(dmax=5.0, hfov=0.7592, vfov=0.4903, is_depth=False, is_spherical=False)

    def call(opts=None, H=h, W=w, scale=0.2, nb=B, p=dp, Rm=dR, img=out, sc=None):
        o = _lib.img_opts(**{**good, **(opts or {})})
        _lib.scene_render(gpu_ctx, scene.h if sc is None else sc, None, o, H, W, scale, nb, p, Rm, img)

    bad = [dict(opts=dict(hfov=np.pi / 2)), dict(opts=dict(vfov=1.6)), dict(opts=dict(dmax=0.0)), dict(opts=dict(dmax=-1.0)),
           dict(opts=dict(hfov=0.0)), dict(opts=dict(vfov=-0.1)), dict(opts=dict(dmax=float("nan"))), dict(scale=0.0),
           dict(H=0), dict(W=0), dict(nb=-1), dict(p=None), dict(Rm=None), dict(img=None), dict(sc=0)]
    for kw in bad:
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            call(**kw)
        gpu_ctx.synchronize()
        np.testing.assert_array_equal(out.numpy(), fill)
    call(nb=0)  # a no-op
    np.testing.assert_array_equal(out.numpy(), fill)
    call(opts=dict(hfov=1.6, vfov=1.0, is_spherical=True))  # a spherical image may be that wide
    assert (out.numpy() >= 0).all()
    # a malformed scene never reaches a launch: it is refused when it is created
    ok = Scene.sphere((1, 0, 0), 0.2)
    for prims in ([ok] * 33, [("sphere", [1, 0, 0, 0.0])], [("sphere", [1, 0, 0, -1.0])], [("box", [0, 0, 0, 1, 0, 1])],
                  [("cylinder", [0, 0, 0.5, 1.0, 1.0])], [("cylinder", [0, 0, 0.0, 0.0, 1.0])], [(7, [0, 0, 0, 1])],
                  [("cone", [0, 0, 0, 1])], [("sphere", [np.inf, 0, 0, 1])]):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            Scene(gpu_ctx, prims)
    Scene(gpu_ctx, [ok] * 32).close()
    # the pose and distance entry points
    x = _lib.DeviceArray.from_numpy(gpu_ctx, np.zeros((2, 10)))
    o3, o9 = _lib.DeviceArray(gpu_ctx, (2, 3)), _lib.DeviceArray(gpu_ctx, (2, 9))
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        _lib.scene_pose(gpu_ctx, np.zeros(3), np.eye(3), -1, x, o3, o9, o3, o9)
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        _lib.scene_pose(gpu_ctx, np.zeros(3), np.eye(3), 2, None, o3, o9, o3, o9)
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        _lib.scene_distance(gpu_ctx, scene.h, None, None, 4, o3)
