"""tests/preproc_ref.py, the numpy restatement of the morphology kernels' semantics, against the reference's own modules
(tests/golden/preproc_golden.npz, written by tests/golden/make_preproc_golden.py): bitwise on every case, and the
quirks the restatement must keep -- Dilate's flipped element over unflipped padding, the border value where every
included tap is padding, inputs left alone."""
import os

import numpy as np
import pytest

import preproc_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preproc_golden.npz")


def golden_cases():
    G = np.load(GOLDEN)
    return G, [str(c) for c in G["cases"]]


def run_case(G, name, dilate, erode, rco):
    """The golden case `name` through an implementation given as dilate(img, kernel, ignore_zeros), erode(...) and
    rco(img, kernel_size, min_range)."""
    op, img = name.split("-")[0], G[f"{name}/img"]
    if op in ("dilate", "erode"):
        return (dilate if op == "dilate" else erode)(img, G[f"{name}/kernel"], name.split("-")[1] == "iz1")
    if op == "open":
        return dilate(erode(img, G[f"{name}/kernel_erode"], False), G[f"{name}/kernel_dilate"], False)
    if op == "close":
        return erode(dilate(img, G[f"{name}/kernel_dilate"], False), G[f"{name}/kernel_erode"], False)
    assert op == "rco"
    return rco(img, 3, 0.1)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_golden_file_is_small_and_complete():
    G, cases = golden_cases()
    assert os.path.getsize(GOLDEN) < 100 * 1024
    assert len(cases) == 25 and len({c.split("-")[0] for c in cases}) == 5
    for c in cases:
        assert G[f"{c}/img"].shape[-2] <= 40 and G[f"{c}/img"].shape[-1] <= 48 and G[f"{c}/img"].dtype == np.float32


@pytest.mark.parametrize("name", golden_cases()[1])
def test_restatement_equals_the_reference_bitwise(name):
    G, _ = golden_cases()
    img = G[f"{name}/img"].copy()
    got = run_case(G, name, PR.dilate, PR.erode, PR.remove_close_outliers)
    assert same_bits(got, G[f"{name}/out"])
    assert same_bits(img, G[f"{name}/img"])  # the restatement leaves its input alone


def test_dilate_scans_the_flipped_element_over_unflipped_padding():
    imp = np.zeros((9, 9), np.float32)
    imp[4, 5] = 1
    assert np.argwhere(PR.dilate(imp, PR.ASYM) > 0).tolist() == [[3, 4], [3, 5], [4, 5], [6, 6]]
    one = np.ones((9, 9), np.float32)
    one[4, 5] = 0
    assert np.argwhere(PR.erode(one, PR.ASYM) == 0).tolist() == [[3, 4], [5, 5], [6, 5], [6, 6]]


def test_border_value_where_every_included_tap_is_padding():
    one = np.ones((9, 9), np.float32)
    e = PR.erode(one, PR.ASYM)
    assert e[0, 8] == 2.0 and (np.delete(e.ravel(), 8) == 1.0).all()  # the top-right pixel: all four taps off the image
    assert (PR.erode(one, PR.ASYM, ignore_zeros=True)[0, 8]) == 0.0  # ... which ignore_zeros turns into 0
    # a dilation there: the excluded taps' bias of -2 is all that is left, as in the reference's module
    d = PR.dilate(np.full((2, 4), 0.5, np.float32), np.array([[1, 0, 0]]))
    assert (d[:, :3] == 0.5).all() and (d[:, 3] == -1.5).all()


def test_refusals_and_shapes():
    with pytest.raises(ValueError):
        PR.dilate(np.ones((3, 3), np.float32), np.zeros((3, 3)))
    a = np.random.default_rng(0).uniform(0, 1, (2, 1, 5, 6)).astype(np.float32)
    assert PR.erode(a, PR.disc(1)).shape == a.shape
    assert same_bits(PR.erode(a, np.ones((1, 1))), a) and same_bits(PR.dilate(a, np.ones((1, 1))), a)
    assert PR.disc(10).shape == (21, 21) and PR.disc(10).sum() == 317
