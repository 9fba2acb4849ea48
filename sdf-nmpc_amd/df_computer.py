"""Distance field implied by depth or range images (the reference's utils/df_computer.py: DfComputer), on the
HIP kernels of csrc/df_truth.hip through the C ABI (sdfnmpc_udf, sdfnmpc_sdf_truth).

Same constructor, methods and defaults as the reference.  Inputs are numpy arrays or torch tensors; the
outputs are torch tensors ``(df [n], grad [n, 3])`` on the computer's device.
"""
from __future__ import annotations

import numpy as np

from .collision_checker import ColChecker, _DeviceSide


class DfComputer:
    """Parallelized signed or unsigned distance function computer from depth or range images.

    As in the reference (df_computer.py:16-17) the clamps are ``min_df = -0.3`` and ``max_df = 1`` whatever
    ``max_df`` is passed.  ``batch_size`` is accepted and unused: the reference needs it to bound its
    points x voxels buffer, which the fused kernel never forms.
    device -- None (cuda:0), a device index / string / torch.device, or an sdf_nmpc_amd Context
    """

    def __init__(self, signed, dmax, hfov, vfov, max_df, is_depth=False, is_spherical=False, batch_size=5000,
                 device=None):
        self.signed = signed
        self.is_depth = is_depth
        self.is_spherical = is_spherical
        self.hfov = hfov
        self.vfov = vfov
        self.dmax = dmax
        self.min_df = -0.3  # assuming min < max
        self.max_df = 1
        self._dev = _DeviceSide(device)
        self._grid_dev = None

        if self.signed:
            self.colcheck = ColChecker(dmax, hfov, vfov, 0, is_depth, is_spherical, 'extrapolate', device=self._dev)
            grid_params = [(0, 0.1, 0.01), (0.1, 0.2, 0.02), (0.2, 0.3, 0.03), (0.3, 0.5, 0.05), (0.5, 1, 0.1)]
            self.batch_size = batch_size
            self.distances, self.grid = self.generate_dist_grid(grid_params)

    @property
    def device(self):
        return self._dev.device

    def generate_dist_grid(self, grid_params):
        """ Compute a voxel grid for computing SDF wrt its center
        The voxel size is typically increasing as the distance to the origin increases for efficiency.
        gris_params is a list of tuples (dmin, dmax, size), such that the grid resolution is, eg:
            0    - 0.05m -> 1cm
            0.05 - 0.1m  -> 2cm
            ...
        Computed with torch float32 on the CPU (df_computer.py:41-57), so the grid is the same everywhere
        (17,652 voxels for the reference's grid_params);
        returns (distances [G], grid [G, 3]) in the reference's order.  The copy the kernel scans is sorted
        by distance (stable) and carries each voxel's index in this order.
        """
        import torch
        distances = torch.tensor([], dtype=torch.float32)
        grid = torch.tensor([], dtype=torch.float32)
        for (dmin, dmax, step) in grid_params:
            nb_points = int(2.*dmax/step) + 1
            # the coordinates are the float32 roundings of the exact linspace (formed in float64): a float32
            # torch.linspace rounds differently on each backend, which moves voxels across the shell borders
            coords = torch.from_numpy(np.linspace(-dmax, dmax, nb_points)).to(torch.float32)
            local_grid = torch.stack([
                coords.repeat(nb_points).repeat(nb_points),
                coords.repeat_interleave(nb_points).repeat(nb_points),
                coords.repeat_interleave(nb_points).repeat_interleave(nb_points),
            ], dim=1)
            local_dist = torch.linalg.norm(local_grid, dim=1)

            idx = (local_dist > dmin) * (local_dist <= dmax)
            grid = torch.cat([grid, local_grid[idx]], dim=0)
            distances = torch.cat([distances, local_dist[idx]], dim=0)

        order = torch.from_numpy(np.argsort(distances.numpy(), kind="stable"))
        self._sorted = (grid[order].contiguous(), distances[order].contiguous(), order.to(torch.int32))
        self._grid_dev = None
        return distances, grid

    def _device_grid(self):
        if self._grid_dev is None:
            self._grid_dev = tuple(t.to(self.device) for t in self._sorted)
        return self._grid_dev

    def get_df(self, imgs, points, p_to_i=None):
        """Compute the signed or unsigned ditance field for points according to imgs.
        Size of image array: [B, H, W] or [H, W].
        Images are assumed normalized wrt dmax.
        Points are unormalized Cartesian coordinates.
        p_to_i is an array mapping each point to the index of the corresponding image (its entries must lie
        in [0, B): they are not checked). If set to None, default ordering is assumed.
        """
        if self.signed:
            return self.get_sdf(imgs, points, p_to_i)
        else:
            return self.get_udf(imgs, points, p_to_i)

    def _opts(self):
        from . import _lib
        return _lib.img_opts(self.dmax, self.hfov, self.vfov, self.is_depth, self.is_spherical)

    def get_udf(self, imgs, points, p_to_i=None, return_index=False):
        """Unsigned distance to the nearest pixel of the 5x5 min-pooled image (zeros skipped) or to the virtual
        wall at dmax, clamped to [0, max_df], and its gradient (df_computer.py:152-182).  H and W must be
        multiples of 5.  return_index: also the pooled pixel chosen (int32 [n])."""
        import torch
        from . import _lib
        imgs, points, p_to_i = self._dev.inputs(imgs, points, p_to_i)
        kernel = 5  # minpool kernel, make sure it divides both dimensions
        assert (imgs.shape[1] % kernel) == 0 and (imgs.shape[2] % kernel) == 0
        n = points.shape[0]
        udf = torch.empty(n, dtype=torch.float32, device=imgs.device)
        grad = torch.empty((n, 3), dtype=torch.float32, device=imgs.device)
        idx = torch.empty(n, dtype=torch.int32, device=imgs.device)
        opts = self._opts()
        self._dev.launch(lambda ctx: _lib.udf(ctx, opts, self.max_df, imgs, points, p_to_i, udf, grad, idx), idx)
        return (udf, grad, idx) if return_index else (udf, grad)

    def get_sdf(self, imgs, points, p_to_i=None, return_index=False, sorted_scan=True):
        """Signed distance over the voxel grid around each point and its gradient (df_computer.py:200-221),
        clamped to [min_df, max_df].  return_index: also the voxel chosen, in generate_dist_grid's order (int32
        [n], -1 where no voxel counts).  sorted_scan False visits every voxel in that order instead of scanning
        the sorted copy with an early stop; the results are bitwise the same."""
        import torch
        from . import _lib
        if not self.signed:
            raise ValueError("get_sdf needs DfComputer(signed=True)")
        imgs, points, p_to_i = self._dev.inputs(imgs, points, p_to_i)
        n = points.shape[0]
        if sorted_scan:
            grid, dist, orig = self._device_grid()
        else:
            grid, dist, orig = self.grid.to(imgs.device), self.distances.to(imgs.device), None
        sdf = torch.empty(n, dtype=torch.float32, device=imgs.device)
        grad = torch.empty((n, 3), dtype=torch.float32, device=imgs.device)
        idx = torch.empty(n, dtype=torch.int32, device=imgs.device)
        opts = self._opts()
        self._dev.launch(lambda ctx: _lib.sdf_truth(ctx, opts, self.min_df, self.max_df, grid, dist, orig, imgs, points,
                                                    p_to_i, sdf, grad, idx), idx)
        return (sdf, grad, idx) if return_index else (sdf, grad)
