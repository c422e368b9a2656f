"""Random parameters of the on-the-fly slice augmentation (DESIGN.md "Augmentation"): host side, numpy only.

The device work is one kernel, pmu_warp_gather (csrc/augment.hip): it samples image and mask of every item
of a batch through a per-item in-plane affine map, a cubic B-spline elastic displacement and an intensity
gain / bias.  This module draws those numbers: nine doubles per item plus 2 G^2 control displacements.

Every item has a generator of its own, a Philox counter stream keyed by (seed, epoch) and started at the
counter (0, scan, view, slice) (word 0 counts the stream's own blocks): an item gets the same warp whatever batch, order, rank or world size serves
it, and a new one every epoch.  Neither torch's default generator (which train.py keeps aligned with the
reference's) nor numpy's global state is touched.
"""
from __future__ import annotations

import numpy as np

# par[b] = [ds, m00, m01, m10, m11, ta, tb, gain, bias]; ds (the slice offset along n) is the dataset's to fill
PAR_LEN = 9
IDENTITY = np.array([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0])
# uniform draws per item ahead of the control grid: apply, angle, scale, mirror, shift a, shift b, gain, bias
_N_AFFINE = 8
# A cubic B-spline displacement field stays free of fold-over while every control displacement is below
# roughly 0.48 of the control spacing; 0.4 leaves a margin.
ELASTIC_MAX = 0.4


class Augment:
    """Random affine + elastic + intensity augmentation of training slices.

    rotate_deg: the in-plane rotation is uniform in [-rotate_deg, rotate_deg] degrees.
    scale: (lo, hi) of the uniform isotropic scale of the sampling grid (> 1 zooms out).
    shift: the translation is uniform in +-shift of the slice extent h (H-1), h (W-1), per axis.
    flip: mirror the second plane axis with probability 1/2.
    elastic: largest control displacement as a fraction of the control spacing h (H-1) / (G-3) (the smaller
      of the two axes' spacings); 0 disables the elastic part (no control grid at all).
    grid: G, the control grid is G x G (4..16).
    gain, bias: the image becomes y (1 + g) + b with g uniform in +-gain, b in +-bias.
    p: probability that an item is augmented at all (else it gets the identity block).
    seed: the stream's seed."""

    def __init__(self, rotate_deg=15, scale=(0.9, 1.1), shift=0.05, flip=False, elastic=0.25, grid=6, gain=0.1,
                 bias=0.05, p=1.0, seed=0):
        if not 0.0 <= elastic <= ELASTIC_MAX:
            raise ValueError(f"elastic must be in [0, {ELASTIC_MAX}] (fold-over beyond ~0.48), got {elastic}")
        if int(grid) != grid or not 4 <= grid <= 16:
            raise ValueError(f"grid must be an integer in 4..16, got {grid}")
        lo, hi = scale
        if not 0.0 < lo <= hi:
            raise ValueError(f"scale must be (lo, hi) with 0 < lo <= hi, got {scale}")
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be a probability, got {p}")
        if int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed}")
        self.rotate_deg, self.scale, self.shift, self.flip = float(rotate_deg), (float(lo), float(hi)), float(shift), bool(flip)
        self.elastic, self.grid, self.gain, self.bias = float(elastic), int(grid), float(gain), float(bias)
        self.p, self.seed = float(p), int(seed)
        self._bg = np.random.Philox(key=np.zeros(2, dtype=np.uint64))

    def _uniforms(self, keys, epoch, n):
        """(B, n) uniforms in [0, 1): row b from the generator keyed by (seed, epoch, *keys[b])."""
        raw = np.empty((len(keys), n), dtype=np.uint64)
        key = np.array([self.seed, int(epoch)], dtype=np.uint64)
        # One bit generator, re-keyed per item: the stream of Philox(key=key, counter=[0, scan, view, slice])
        # (word 0 is the running block count), at half the host time of constructing one per item.
        bg = self._bg
        st = bg.state
        st["state"]["key"], st["buffer_pos"], st["has_uint32"] = key, 4, 0
        for b, (scan, view, sl) in enumerate(keys):
            st["state"]["counter"] = np.array([0, scan, view, sl], dtype=np.uint64)
            bg.state = st
            raw[b] = bg.random_raw(n)
        return (raw >> np.uint64(11)) * (1.0 / 9007199254740992.0)   # 53-bit uniforms, as Generator.random

    def draw(self, keys, epoch, H, W, h):
        """Parameter blocks of the items ``keys`` ((scan, view, slice) triples) in ``epoch`` for H x W slices
        at spacing h: (par (B, 9) float64 with par[:, 0] = 0 for the dataset to fill, ctrl (B, 2, G, G) float64
        plane displacements in voxels, or None when elastic == 0)."""
        B, G = len(keys), self.grid
        elastic = self.elastic > 0.0
        u = self._uniforms(keys, epoch, _N_AFFINE + (2 * G * G if elastic else 0))
        on = u[:, 0] < self.p
        theta = np.deg2rad((2.0 * u[:, 1] - 1.0) * self.rotate_deg)
        lo, hi = self.scale
        s = lo + u[:, 2] * (hi - lo)
        mirror = np.where(self.flip & (u[:, 3] < 0.5), -1.0, 1.0)
        c, sn = np.cos(theta) * s, np.sin(theta) * s
        par = np.empty((B, PAR_LEN))
        par[:, 0] = 0.0
        par[:, 1], par[:, 2] = c, -sn * mirror          # M = R(theta) diag(s, s) diag(1, mirror)
        par[:, 3], par[:, 4] = sn, c * mirror
        par[:, 5] = (2.0 * u[:, 4] - 1.0) * (self.shift * h * (H - 1))
        par[:, 6] = (2.0 * u[:, 5] - 1.0) * (self.shift * h * (W - 1))
        par[:, 7] = 1.0 + (2.0 * u[:, 6] - 1.0) * self.gain
        par[:, 8] = (2.0 * u[:, 7] - 1.0) * self.bias
        par[~on] = IDENTITY
        par += 0.0                                        # no negative zeros: zero strength is the identity block
        if not elastic:
            return par, None
        spacing = h * (min(H, W) - 1) / (G - 3)
        ctrl = (2.0 * u[:, _N_AFFINE:] - 1.0).reshape(B, 2, G, G) * (self.elastic * spacing)
        ctrl[~on] = 0.0
        return par, ctrl
