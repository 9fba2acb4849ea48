"""Regenerates tests/golden/preproc_golden.npz: inputs and expected outputs of the reference's morphology modules.

    python tests/golden/make_preproc_golden.py <path of the reference checkout>

The reference's utils/preprocessing.py is loaded as a file (it imports numpy and torch only) and run with torch on
the CPU.  Cases (names in the array ``cases``; ``<case>/img``, ``<case>/out`` and the element(s) per case):

  dilate|erode - iz0|iz1 - <element>   Dilate / Erode with ignore_zeros off / on; ``<case>/kernel``.  Elements: ones3
                                       (3 x 3 of ones) on [2, 12, 19]; asym (the 4 x 3 element of tests/preproc_ref.py,
                                       even-sized and asymmetric: the flip shows) on [1, 23, 30]; disc3 (radius 3) on
                                       [2, 1, 15, 18]; disc10 (21 x 21) on [1, 3, 2], an image smaller than the element
  open|close - patches|zeros|ones      Open / Close with ``<case>/kernel_erode`` = ones3, ``<case>/kernel_dilate`` = a
                                       3 x 3 cross, on an image with zero patches, all zeros, all ones ([1, 14, 17])
  rco - patches|zeros|ones             RemoveCloseOutliers(3, 0.1) on the same images (the patch image also has values
                                       below min_range and isolated pixels)

Every module gets a clone (Dilate / Erode with ignore_zeros overwrite their input).  Arrays only are written.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import preproc_ref as PR  # noqa: E402  (the elements only)


def reference_preprocessing(ref_root):
    spec = importlib.util.spec_from_file_location("ref_preprocessing",
                                                  os.path.join(ref_root, "sdf_nmpc", "utils", "preprocessing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def patch_image(rng, shape):
    """Values in [0, 1] with rectangular zero patches, a few isolated survivors inside them and a few short values."""
    a = rng.uniform(0.15, 1.0, shape).astype(np.float32)
    H, W = shape[-2:]
    flat = a.reshape(-1, H, W)
    for im in flat:
        for _ in range(3):
            y, x = rng.integers(0, H - 3), rng.integers(0, W - 3)
            h, w = rng.integers(2, 6), rng.integers(2, 7)
            keep = im[y + 1, x + 1]
            im[y:y + h, x:x + w] = 0.0
            im[y + 1, x + 1] = keep  # an isolated pixel in the shadow: what RemoveCloseOutliers removes
        idx = rng.integers(0, H * W, 6)
        im.reshape(-1)[idx] = rng.uniform(0.0, 0.1, 6).astype(np.float32)  # below min_range
    return a


def main(ref_root):
    P = reference_preprocessing(ref_root)
    rng = np.random.default_rng(20240611)
    out, cases = {}, []
    run = lambda mod, img: mod(torch.from_numpy(img).clone()).numpy()
    elements = {"ones3": (np.ones((3, 3), np.uint8), (2, 12, 19)), "asym": (PR.ASYM, (1, 23, 30)),
                "disc3": (PR.disc(3), (2, 1, 15, 18)), "disc10": (PR.disc(10), (1, 3, 2))}
    for ename, (k, shape) in elements.items():
        img = patch_image(rng, shape) if ename != "disc10" else np.array([[[0.5, 0.0], [0.25, 0.75], [0.0, 1.0]]], np.float32)
        for op, cls in (("dilate", P.Dilate), ("erode", P.Erode)):
            for iz in (0, 1):
                name = f"{op}-iz{iz}-{ename}"
                cases.append(name)
                out[f"{name}/img"], out[f"{name}/kernel"] = img, k
                out[f"{name}/out"] = run(cls(k.astype(np.float64), bool(iz)), img)
                assert np.array_equal(out[f"{name}/img"], img)
    ones3, cross = np.ones((3, 3), np.uint8), np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
    images = {"patches": patch_image(rng, (1, 14, 17)), "zeros": np.zeros((1, 14, 17), np.float32),
              "ones": np.ones((1, 14, 17), np.float32)}
    for iname, img in images.items():
        for op, cls in (("open", P.Open), ("close", P.Close)):
            name = f"{op}-{iname}"
            cases.append(name)
            out[f"{name}/img"], out[f"{name}/kernel_erode"], out[f"{name}/kernel_dilate"] = img, ones3, cross
            out[f"{name}/out"] = run(cls(ones3.astype(np.float64), cross.astype(np.float64)), img)
        name = f"rco-{iname}"
        cases.append(name)
        out[f"{name}/img"] = img
        out[f"{name}/out"] = run(P.RemoveCloseOutliers(3, 0.1), img)
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "preproc_golden.npz")
    np.savez_compressed(path, **out)
    print(f"preproc_golden.npz: {len(cases)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
