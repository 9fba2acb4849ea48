"""The CPU side of the sensor stage: tests/sensor_ref.py's Philox4x32-10 against the Random123 known-answer vectors,
the oracle's own noise statistics for the seed the GPU test uses, and the contract of the box-table generator
(sdf_nmpc_amd.sensor.box_table)."""
import numpy as np
import pytest

import sensor_ref as SR
from sdf_nmpc_amd.sensor import box_table

STAT_SEED, STAT_SHAPE = 0x5EED0123456789AB, (3, 18, 32)  # the noise-statistics case of tests/test_gpu_sensor.py


@pytest.mark.parametrize("ctr,key,want", SR.KAT)
def test_philox_known_answers(ctr, key, want):
    got = SR.philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == want


def test_philox_is_elementwise():
    c = np.arange(12, dtype=np.uint32).reshape(3, 4)
    w = SR.philox4x32_10(c, 7, c.T[:1].T, 0, 0xdeadbeef, 0x12345678)
    for i in range(3):
        for j in range(4):
            one = SR.philox4x32_10(int(c[i, j]), 7, int(c[i, 0]), 0, 0xdeadbeef, 0x12345678)
            assert [int(v[i, j]) for v in w] == [int(v) for v in one]


def noise_statistics(z):
    """(|mean|, |variance - 1|, their five-standard-error bounds 5 / sqrt(n) and 5 sqrt(2 / n))."""
    n = z.size
    return abs(z.mean()), abs(z.var() - 1.0), 5.0 / np.sqrt(n), 5.0 * np.sqrt(2.0 / n)


def test_oracle_noise_statistics_hold_for_the_gpu_tests_seed():
    B, H, W = STAT_SHAPE
    _, _, z = SR.degrade(np.ones(STAT_SHAPE), STAT_SEED, 3, a=0.125, vmax=100.0)
    m, v, bm, bv = noise_statistics(z)
    assert m <= bm and v <= bv, (m, v, bm, bv)
    assert np.abs(z).max() <= np.sqrt(-2.0 * np.log(2.0**-24))


def test_oracle_degradation_order_and_masks():
    rng = np.random.default_rng(1)
    img = rng.uniform(0.3, 0.9, (2, 7, 13))
    img[0, 2, 3] = 0.0   # already invalid
    img[1, 4, 5] = 1.0   # at vmax: a miss
    tab = np.zeros((1, 2, 2, 4), np.int16)
    tab[0, 1, 0] = (1, 2, 3, 4)
    out, zero, z = SR.degrade(img, 9, 0, a=0.01, vmax=1.0, p_thresh=int(0.2 * 2**32), miss_invalid=True, table=tab)
    assert zero[0, 2, 3] and zero[1, 4, 5] and zero[1, 1:4, 2:6].all() and not zero[0, 1:4, 2:6].all()
    assert (out[zero] == 0).all() and (out[~zero] > 0).all()
    keep = ~zero
    np.testing.assert_allclose(out[keep], np.clip(img[keep] + 0.01 * z[keep], 0, 1), rtol=0, atol=0)
    frac = (SR.words(9, 0, [0, 1], 7, 13)[2] < np.uint32(int(0.2 * 2**32))).mean()
    assert 0.05 < frac < 0.4  # about a fifth of the pixels are dropped
    clean, zero0, _ = SR.degrade(img, 9, 0, vmax=1.0)
    assert np.array_equal(clean, img) and np.array_equal(zero0, img == 0)


@pytest.mark.parametrize("H,W", [(7, 13), (18, 32)])
def test_box_table_contract(H, W):
    kw = dict(p_box=0.6, n_min=2, n_max=4, scale=(0.02, 0.06), ratio=(0.2, 5.0))
    streams = [5, 0, 5]
    t = box_table(77, streams, 40, H, W, **kw)
    assert t.shape == (40, 3, 4, 4)
    count = SR.check_box_table(t, H, W, kw["n_min"], kw["n_max"], kw["p_box"])
    # at these sizes every drawn box fits, so an entry holds none or n_min..n_max boxes; both happen
    assert ((count == 0) | ((count >= kw["n_min"]) & (count <= kw["n_max"]))).all()
    assert (count == 0).any() and (count > 0).any()
    assert np.array_equal(t, box_table(77, streams, 40, H, W, **kw))        # the same seed, the same table
    assert not np.array_equal(t, box_table(78, streams, 40, H, W, **kw))
    assert np.array_equal(t[:, 0], t[:, 2]) and not np.array_equal(t[:, 0], t[:, 1])  # an entry follows its stream
    assert np.array_equal(t[:, 1:2], box_table(77, [0], 40, H, W, **kw))    # ... and not the batch around it
    empty = box_table(77, streams, 40, H, W, **dict(kw, p_box=0.0))
    assert SR.check_box_table(empty, H, W, 2, 4, 0.0).sum() == 0 and not empty.any()
    m = SR.box_mask(t, 43, 3, H, W)  # frame 43 reads entry 43 % 40
    assert np.array_equal(m, SR.box_mask(t[3:4], 0, 3, H, W)) and m.any()


def test_box_table_refusals_and_skips():
    with pytest.raises(ValueError):
        box_table(1, [0], 1, 18, 32, n_max=9)
    with pytest.raises(ValueError):
        box_table(1, [0], 1, 18, 32, scale=(0.0, 0.1))
    # boxes that can never fit (area fraction ~1 of a 4 x 4 image) are skipped after ten draws: an empty table
    assert not box_table(1, [0, 1], 8, 4, 4, p_box=1.0, scale=(1.5, 2.0), ratio=(1.0, 1.0)).any()
