"""numpy oracle of the sensor-degradation stage (csrc/sensor.hip, sdfnmpc_sensor_apply): Philox4x32-10, the
degradation restated in float64 on the same uniforms, and the contract of the box-table generator
(sdf_nmpc_amd.sensor.box_table).

Philox4x32-10 is defined by its round constants (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
0xBB67AE85) and pinned to the Random123 known-answer vectors KAT below (tests/test_sensor_ref.py); all three agree
with this implementation.

The noise tolerance Z_TOL.  The device forms z = sqrtf(-2 logf(u1)) cosf(2 pi u2) in fp32; the oracle forms it in
float64 from the same u1, u2 (exact in both).  A test recovers the device's z from a constant image as (v' - v) / a
with v = 1 and a = 2^-3, which adds the rounding of v' = fl(v + a z) in [0.25, 1.75], at most 2^-24 / a = 4.8e-7.
Measured on an MI355X at 7 x 13 and 18 x 32, B = 3, frames 0, 3 and 11: max |z_dev - z_ref| = MEASURED_Z_ERR = 1.40e-6
(1.46e-6 at 64 x 64).  Z_TOL is four times that, to absorb another math-library build, and stays under the 1e-5 that
fp32 rounding allows (2 pi u2 rounded to <= 2^-22 absolute in the angle, a few ulp in logf and cosf, |r| <= sqrt(-2 ln
2^-24) = 5.77): a larger error is a wrong formula, not rounding.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KAT = [  # counter, key -> output (Random123 kat_vectors, philox4x32 10 rounds)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

MEASURED_Z_ERR = 1.40e-6  # tests/test_gpu_sensor.py prints the figure of its own run
Z_TOL = 4 * MEASURED_Z_ERR
Z_TOL_MAX = 1e-5


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of uint32 words, broadcast together -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def words(seed, frame, stream_id, H, W):
    """The four Philox words of every pixel: [B][H][W] each, the counter (y W + x, frame, stream_id[b], 0), the
    key (seed's low word, high word)."""
    pix = np.arange(H * W, dtype=np.uint64).reshape(1, H, W)
    st = (np.asarray(stream_id, dtype=np.int64) & 0xffffffff).reshape(-1, 1, 1)
    seed = int(seed) & (2**64 - 1)
    return philox4x32_10(pix, int(frame), st, 0, seed & 0xffffffff, seed >> 32)


def normal(w0, w1):
    """Box-Muller in float64 on the uniforms u = ((w >> 8) + 1) 2^-24 in (0, 1]."""
    u1 = ((w0 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0**-24
    u2 = ((w1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0**-24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def box_mask(table, frame, B, H, W):
    """bool [B][H][W]: inside an erased box of frame % n_frames (table [n_frames][B][max_boxes][4] or None)."""
    m = np.zeros((B, H, W), bool)
    if table is None:
        return m
    for b in range(B):
        for y0, x0, h, w in table[int(frame) % table.shape[0], b]:
            m[b, y0:y0 + h, x0:x0 + w] = True  # h == 0: nothing
    return m


def degrade(img, seed, frame, stream_id=None, a=0.0, b=0.0, vmax=1.0, p_thresh=0, miss_invalid=False, table=None):
    """The degradation of img [B][H][W] in float64.  Returns (out float64, zero bool, z float64): zero is the mask of
    the integer decisions alone (already 0, miss, dropout, box) -- not a pixel the noise happens to clamp to 0."""
    v = np.asarray(img, dtype=np.float64).copy()
    B, H, W = v.shape
    st = np.arange(B) if stream_id is None else stream_id
    w0, w1, w2, _ = words(seed, frame, st, H, W)
    if miss_invalid:
        v[v >= vmax] = 0.0
    z = normal(w0, w1)
    valid = v != 0.0
    v = np.where(valid, np.clip(v + (a + b * v * v) * z, 0.0, vmax), 0.0)
    zero = ~valid | (w2 < np.uint32(p_thresh)) | box_mask(table, frame, B, H, W)
    v[zero] = 0.0
    return v, zero, z


def check_box_table(table, H, W, n_min, n_max, p_box):
    """The generator's contract: int16 [n_frames][B][max_boxes][4]; every box (h > 0) lies inside the image with 0 <
    h < H and 0 < w < W; the boxes of an entry fill its first slots; an entry holds none or at most n_max (a box that
    never fits is skipped, so fewer than n_min may remain); p_box == 0 gives none at all."""
    assert table.dtype == np.int16 and table.ndim == 4 and table.shape[-1] == 4
    y0, x0, h, w = (table[..., i].astype(int) for i in range(4))
    on = h > 0
    assert ((w > 0) == on).all() and (table[~on] == 0).all()
    assert (y0[on] >= 0).all() and (x0[on] >= 0).all() and (y0[on] + h[on] <= H).all() and (x0[on] + w[on] <= W).all()
    assert (h[on] < H).all() and (w[on] < W).all()
    count = on.sum(-1)
    assert (count <= n_max).all()
    assert (on[..., :-1] >= on[..., 1:]).all()  # filled from the first slot
    if p_box == 0:
        assert count.max(initial=0) == 0
    return count
