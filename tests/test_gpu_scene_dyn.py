"""The dynamic kernels of csrc/scene.hip (primitives with a frame that is a function of time) against
tests/scene_dyn_ref.py, against the static kernels where a motion can be undone by hand, and the contract that a static
scene keeps its kernel and its bits whatever time it is given.

The image bar, 1e-4 m, is the static test's with the same derivation: on a decided ray the discriminant is bounded away
from zero, b^2 and c are at most dmax^2 = 25, so the fp32 discriminant error is about 1e-5 and the root error that
divided by 2 sqrt(disc); the frame, formed in fp64 and rounded to fp32 once, adds about 1e-6 (coordinates of a few
metres times 2^-24, through the direction and the origin)."""
import numpy as np
import pytest

import scene_dyn_ref as D
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


def _prims(spec=D.SPEC):
    """The fixture through the public constructor (rpy -> quaternion happens in the package)."""
    return [Scene.moving(p, **kw) if kw is not None else p for p, kw in spec]


@pytest.fixture(scope="module")
def scene(gpu_ctx):
    return Scene(gpu_ctx, _prims())


@pytest.fixture(scope="module")
def static(gpu_ctx):
    return Scene(gpu_ctx, R.SCENE)


@pytest.fixture(scope="module")
def ref():
    """Reference values in metres and decided masks [T, B, h, w], once per (sensor, shape, is_depth)."""
    cache, prims = {}, D.scene()

    def get(sensor, shape, is_depth):
        key = (sensor, tuple(shape), bool(is_depth))
        if key not in cache:
            s = R.SENSOR if sensor == "pinhole" else R.SPHERICAL
            kw = dict(is_depth=is_depth, is_spherical=sensor == "spherical")
            v = np.stack([D.values(prims, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], t, **kw) for t in D.TIMES])
            ok = np.stack([D.decided(prims, P, RM, *shape, s["hfov"], s["vfov"], s["dmax"], t, **kw) for t in D.TIMES])
            v.setflags(write=False)
            ok.setflags(write=False)
            cache[key] = (v, ok)
        return cache[key]

    return get


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("sensor", ["pinhole", "spherical"])
def test_render_matches_reference_on_decided_pixels(scene, ref, sensor, shape):
    """Times 0, 0.7 and 2.3; range and depth, normalised and raw (mm_resolution = 250: four units per metre), B = 3."""
    assert scene.is_dynamic
    worst = 0.0
    for is_depth in (False, True):
        cfg = _cfg(sensor, is_depth, sensor__mm_resolution=250)
        want, ok = ref(sensor, shape, is_depth)
        assert ok.reshape(len(D.TIMES) * B, -1).mean(1).min() >= 0.98
        for k, t in enumerate(D.TIMES):
            for normalized, per_metre in ((True, 1.0 / 5.0), (False, 4.0)):
                img = scene.render(P, RM, cfg, shape, normalized=normalized, t=t).numpy()
                assert img.shape == (B,) + tuple(shape) and img.dtype == np.float32
                gap = np.abs(img.astype(np.float64) / per_metre - want[k])
                print(f"\n{sensor} {shape} t={t} depth={is_depth} normalized={normalized}: worst gap on decided "
                      f"pixels {gap[ok[k]].max():.3e} m, on all pixels {gap.max():.3e} m")
                worst = max(worst, gap[ok[k]].max())
                assert gap[ok[k]].max() <= IMG_ATOL
                assert img.max() <= np.float32(5.0 * per_metre)
        # without t the scene is shown at t = 0
        np.testing.assert_array_equal(scene.render(P, RM, cfg, shape).numpy(), scene.render(P, RM, cfg, shape, t=0.0).numpy())
    print(f"\n{sensor} {shape}: worst gap {worst:.3e} m")
    assert (np.abs(want[0] - want[2]) > 0.1).mean() > 0.2  # the scene moves


def test_static_scene_keeps_its_bits(gpu_ctx, static):
    """A time does not reach a static scene's kernel, and default motions do not make a scene dynamic."""
    assert not static.is_dynamic
    wrapped = Scene(gpu_ctx, [Scene.moving(p) for p in R.SCENE])
    mixed = Scene(gpu_ctx, [Scene.moving(R.SCENE[0], q=(-3.0, 0, 0, 0), rpy=None, omega=2.0, phase=1.0)] + R.SCENE[1:])
    assert not wrapped.is_dynamic and not mixed.is_dynamic
    for sensor, is_depth in (("pinhole", False), ("spherical", True)):
        cfg = _cfg(sensor, is_depth)
        want = static.render(P, RM, cfg, (27, 48)).numpy()
        np.testing.assert_array_equal(static.render(P, RM, cfg, (27, 48), t=1.7).numpy(), want)
        np.testing.assert_array_equal(wrapped.render(P, RM, cfg, (27, 48)).numpy(), want)
        np.testing.assert_array_equal(wrapped.render(P, RM, cfg, (27, 48), t=1.7).numpy(), want)
        np.testing.assert_array_equal(mixed.render(P, RM, cfg, (27, 48), t=0.4).numpy(), want)


def test_translation_equals_shifted_primitives_and_shifted_camera(gpu_ctx, static):
    """v t undone by hand: the static kernel on primitives shifted by v t, and on the unshifted scene from a camera
    shifted by -v t.  Both within the image bar on the pixels decided in the shifted static scene."""
    v, t = np.array([0.3, -0.4, 0.15]), 1.3
    sh = v * t
    moving = Scene(gpu_ctx, [Scene.moving(p, v=v) for p in R.SCENE])
    assert moving.is_dynamic

    def shifted(kind, a):
        a = np.array(a, float)
        idx = {"sphere": ([0, 1, 2],), "box": ([0, 1, 2], [3, 4, 5]), "cylinder": ([0, 1], )}[kind]
        for ix in idx:
            a[ix] += sh[:len(ix)]
        if kind == "cylinder":
            a[3:5] += sh[2]
        return (kind, list(a))

    prims = [shifted(k, a) for k, a in R.SCENE]
    s = R.SENSOR
    for is_depth in (False, True):
        cfg = _cfg("pinhole", is_depth)
        ok = R.decided(prims, P, RM, 27, 48, s["hfov"], s["vfov"], s["dmax"], is_depth=is_depth)
        assert ok.mean() >= 0.98
        got = moving.render(P, RM, cfg, (27, 48), t=t).numpy().astype(np.float64) * 5.0
        a = Scene(gpu_ctx, prims).render(P, RM, cfg, (27, 48)).numpy().astype(np.float64) * 5.0
        b = static.render(P - sh, RM, cfg, (27, 48)).numpy().astype(np.float64) * 5.0
        print(f"\ndepth={is_depth}: against shifted primitives {np.abs(got - a)[ok].max():.3e} m, against a shifted "
              f"camera {np.abs(got - b)[ok].max():.3e} m")
        assert np.abs(got - a)[ok].max() <= IMG_ATOL
        assert np.abs(got - b)[ok].max() <= IMG_ATOL
        assert np.abs(got - static.render(P, RM, cfg, (27, 48)).numpy() * 5.0).max() > 0.1


def test_capacity_scene_sets_and_batch_independence(gpu_ctx, scene):
    cfg = _cfg("pinhole", True)
    t = 0.7
    # 32 moving primitives in one scene, against the reference
    rng = np.random.default_rng(8)
    spec = []
    for i in range(32):
        c = np.array([rng.uniform(2.0, 4.5), rng.uniform(-2.0, 2.0), rng.uniform(-1.0, 1.0)])
        prim = [("sphere", [*c, 0.3]), ("box", [*(c - 0.25), *(c + 0.25)]),
                ("cylinder", [c[0], c[1], 0.2, c[2] - 0.4, c[2] + 0.4])][i % 3]
        spec.append((prim, dict(v=tuple(rng.uniform(-0.3, 0.3, 3)), rpy=tuple(rng.uniform(-1, 1, 3)), yaw_rate=rng.uniform(-1, 1))))
    full = Scene(gpu_ctx, _prims(spec))
    s = R.SENSOR
    want = D.values(D.scene(spec), P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], t, is_depth=True)
    ok = D.decided(D.scene(spec), P, RM, 18, 32, s["hfov"], s["vfov"], s["dmax"], t, is_depth=True)
    got = full.render(P, RM, cfg, (18, 32), t=t).numpy().astype(np.float64) * 5.0
    print(f"\n32 primitives: {100 * ok.mean():.1f} % decided, worst gap {np.abs(got - want)[ok].max():.3e} m")
    assert ok.reshape(B, -1).mean(1).min() >= 0.98 and (want < 5.0).mean() > 0.25
    assert np.abs(got - want)[ok].max() <= IMG_ATOL
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        Scene(gpu_ctx, _prims(spec + spec[:1]))
    # a set of a static and a dynamic scene: every instance sees its own scene (the set is dynamic: one kernel)
    so = [1, 0, 1]
    both = Scene(gpu_ctx, [R.SCENE, _prims()], scene_of=so)
    assert both.is_dynamic
    img = both.render(P, RM, cfg, (27, 48), t=t).numpy()
    own = [Scene(gpu_ctx, [R.SCENE, _prims()], scene_of=[k] * B).render(P, RM, cfg, (27, 48), t=t).numpy() for k in (0, 1)]
    for b, k in enumerate(so):
        np.testing.assert_array_equal(img[b], own[k][b])
    assert np.abs(own[0] - own[1]).max() > 0.1
    np.testing.assert_array_equal(own[1], scene.render(P, RM, cfg, (27, 48), t=t).numpy())
    # the static member through the dynamic kernel is the static kernel's image to the bar
    sok = R.decided(R.SCENE, P, RM, 27, 48, s["hfov"], s["vfov"], s["dmax"], is_depth=True)
    gap = np.abs(own[0].astype(np.float64) - Scene(gpu_ctx, R.SCENE).render(P, RM, cfg, (27, 48)).numpy()) * 5.0
    assert gap[sok].max() <= IMG_ATOL
    # permutation, and a batch of one
    perm = [2, 0, 1]
    np.testing.assert_array_equal(scene.render(P[perm], RM[perm], cfg, (27, 48), t=t).numpy(), own[1][perm])
    np.testing.assert_array_equal(scene.render(P[1:2], RM[1:2], cfg, (27, 48), t=t).numpy()[0], own[1][1])


def test_camera_inside_the_rotated_box_sees_zero(gpu_ctx):
    """The unit box about (3, 0, 0) turning at pi / 8 per second: at t = 2 it is yawed by pi / 4 and holds the point
    (3.6, 0, 0), which lies outside it at t = 0."""
    box = Scene(gpu_ctx, [Scene.moving(Scene.box((2.5, -0.5, -0.5), (3.5, 0.5, 0.5)), yaw_rate=np.pi / 8)])
    cfg = _cfg()
    p = np.tile([3.6, 0.0, 0.0], (B, 1))
    assert not box.render(p, RM, cfg, (18, 32), normalized=False, t=2.0).numpy().any()
    assert box.render(p, RM, cfg, (18, 32), normalized=False, t=0.0).numpy().all()
    np.testing.assert_allclose(box.distance(p[:1], t=2.0), -(0.5 - 0.6 / np.sqrt(2)), atol=1e-12)


def test_distance_matches_reference(gpu_ctx, scene, static):
    rng = np.random.default_rng(4)
    pts = rng.uniform([-1, -3, -2.5], [6, 3, 2.5], (700, 3))  # three blocks; inside and outside every primitive
    times = rng.uniform(0.0, 3.0, 700)
    want = D.distance(D.scene(), pts, times)
    assert (want < 0).sum() > 20 and (want > 0).sum() > 300
    got = scene.distance(pts, t=times)
    print(f"\ndistance with per-point times: max error {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(want - D.distance(D.scene(), pts, 0.0)).max() > 0.1
    assert np.abs(scene.distance(pts, t=2.3) - D.distance(D.scene(), pts, 2.3)).max() <= 1e-12
    np.testing.assert_array_equal(scene.distance(pts), scene.distance(pts, t=0.0))
    np.testing.assert_array_equal(scene.distance(pts), scene.distance(pts, t=np.zeros(700)))
    # a static scene with times: the static kernel's bits
    np.testing.assert_array_equal(static.distance(pts, t=times), static.distance(pts))
    # two scenes, one of them static: p_to_scene and the default ordering
    both = Scene(gpu_ctx, [R.SCENE, _prims()])
    p2s = rng.integers(0, 2, 700)
    w0 = R.distance(R.SCENE, pts)
    assert np.abs(both.distance(pts, p2s, t=times) - np.where(p2s == 1, want, w0)).max() <= 1e-12
    assert np.abs(both.distance(pts, t=times) - np.where(np.arange(700) >= 350, want, w0)).max() <= 1e-12


def test_refusals_leave_the_output_untouched(gpu_ctx, scene):
    h, w = 18, 32
    fill = np.full((B, h, w), -7.0, np.float32)
    out = _lib.DeviceArray.from_numpy(gpu_ctx, fill)
    cfg = _cfg()
    sph = Scene.sphere((2.0, 0.0, 0.0), 0.5)
    with pytest.raises(ValueError):
        Scene.moving(sph, q=(1, 0, 0, 0), rpy=(0, 0, 0))
    for kw in (dict(q=(0.0, 0.0, 0.0, 0.0)), dict(v=(0.0, float("nan"), 0.0)), dict(q=(1.0, float("inf"), 0, 0)),
               dict(amp=(float("inf"), 0, 0)), dict(yaw_rate=float("nan")), dict(omega=float("inf")),
               dict(phase=float("nan"))):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            Scene(gpu_ctx, [R.SCENE[1], Scene.moving(sph, **kw)])
    # the checks a plain scene gets still apply to a scene with motions
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        Scene(gpu_ctx, [Scene.moving(("sphere", [1, 0, 0, -1.0]), v=(1, 0, 0))])
    for t in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.SdfnmpcError, match="error -1"):
            scene.render(P, RM, cfg, (h, w), out=out, t=t)
        gpu_ctx.synchronize()
        np.testing.assert_array_equal(out.numpy(), fill)
    dp = _lib.DeviceArray.from_numpy(gpu_ctx, P)
    dR = _lib.DeviceArray.from_numpy(gpu_ctx, RM.reshape(B, 9))
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):  # what the static entry point refuses, _at refuses
        _lib.scene_render_at(gpu_ctx, scene.h, None, _lib.img_opts(5.0, 0.0, 0.4903, False, False), h, w, 0.2, B, dp, dR,
                             0.5, out)
    gpu_ctx.synchronize()
    np.testing.assert_array_equal(out.numpy(), fill)
    pts = np.zeros((6, 3))
    for t in (np.zeros(5), np.zeros(7), np.array([0, 0, np.nan, 0, 0, 0]), float("inf")):
        with pytest.raises(ValueError):
            scene.distance(pts, t=t)
    dout = _lib.DeviceArray.from_numpy(gpu_ctx, np.full(6, -7.0))
    with pytest.raises(_lib.SdfnmpcError, match="error -1"):
        _lib.scene_distance_at(gpu_ctx, scene.h, None, None, None, 6, dout)
    np.testing.assert_array_equal(dout.numpy(), np.full(6, -7.0))
    scene.render(P, RM, cfg, (h, w), out=out, t=0.5)  # and it still runs
    assert (out.numpy() >= 0).all()
