"""Seeded inputs of the block-matching tests, and the seam table of csrc/bm.hip read from bm_plan.hip.h's constants: image sizes
at which the matching kernel's tile of band columns and band of rows end one short of, at, and one past a seam."""
from __future__ import annotations

import functools
import pathlib
import re

import numpy as np

import bm_numpy as bn

ROOT = pathlib.Path(__file__).resolve().parents[1]
PLAN = ROOT / "ros_stereo_slam_amd" / "csrc" / "bm_plan.hip.h"


@functools.lru_cache(None)
def plan_constants() -> dict:
    text = PLAN.read_text()
    out = {}
    for name in ("MAX_W", "MAX_PAIRS", "MAX_D", "MIN_BLOCK", "MAX_BLOCK", "MAX_CAP", "THREADS", "BAND", "TX_MAX", "TX_MIN"):
        m = re.search(rf"\b{name} = (\d+)", text)
        assert m, name
        out[name] = int(m.group(1))
    m = re.search(r"LDS_BUDGET = (\d+) \* 1024", text)
    out["LDS_BUDGET"] = int(m.group(1)) * 1024
    return out


def _align16(b):
    return (b + 15) & ~15


def lds_bytes(tx: int, D: int, block: int) -> int:
    """bm_plan::lds(tx, D, block).total, restated (tests/cpp/bm_plan_check.cpp prints the plan's own table; test_bm_abi compares)."""
    k = plan_constants()
    ue = tx + block - 1
    rw = ue + D - 1
    off = _align16(ue * D * 2)
    off = _align16(off + tx * (D + k["THREADS"] // tx) * 4)
    off = _align16(off + ue * 4)
    return _align16(off + 2 * ue + 2 * rw)


def tile_width(D: int, block: int) -> int:
    k = plan_constants()
    tx = k["TX_MAX"]
    while tx > k["TX_MIN"] and lds_bytes(tx, D, block) > k["LDS_BUDGET"]:
        tx //= 2
    return tx


def width_for_band(p: bn.Params, band_columns: int) -> int:
    """The image width whose band has exactly this many columns with a pixel."""
    for w in range(1, 4096):
        if not bn.empty_band(p, w):
            lofs, _, width1 = bn.geometry(p, w)
            if min(width1, w - lofs) == band_columns:
                return w
    raise AssertionError


def seam_sizes(p: bn.Params):
    """(w, h) at the seams of the kernel for these parameters: tile width - 1, + 0, + 1, two tiles + 1, a one-column band;
    band height - 1, + 0, + 1, h = block_size, an odd h."""
    k = plan_constants()
    tx, band, b = tile_width(p.num_disparities, p.block_size), k["BAND"], p.block_size
    hh = max(b, 12)
    sizes = [(width_for_band(p, n), hh) for n in (tx - 1, tx, tx + 1, 2 * tx + 1)]
    sizes += [(width_for_band(p, tx // 2 + 3), h) for h in (band - 1, band, band + 1, b, b + (b + 1) % 2 + 2)]
    w1 = width_for_band(p, 1)
    if w1 >= b:                      # block_size <= min(w, h)
        sizes.append((w1, hh))
    return [(w, h) for w, h in sizes if w >= b and h >= b]


def textured_pair(w: int, h: int, c: int = 1, shift: int = 4, seed: int = 0, flat: bool = True):
    """A smoothed random texture seen from two columns `shift` apart, noise of a few grey levels on the right view, a constant
    patch (texture test) and a repeated pattern (uniqueness test) when `flat`.  -> (left, right) uint8 h x w (x c)."""
    rng = np.random.default_rng(1000 + seed)
    base = rng.integers(0, 256, (h, w + shift + 8, c)).astype(np.float32)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0) + np.roll(base, -1, 1)) / 4
    if flat and h >= 12 and w >= 40:
        base[h // 4:h // 4 + h // 3, w // 2:w // 2 + w // 4] = 90
        per = base[:, 4:10].copy()
        for k in range(w // 8, w // 8 + 24, 6):
            base[h // 2:, k:k + 6] = per[h // 2:]
    L = base[:, 4:4 + w]
    R = base[:, 4 + shift:4 + shift + w] + rng.integers(-3, 4, (h, w, c))
    L, R = np.clip(L, 0, 255).astype(np.uint8), np.clip(R, 0, 255).astype(np.uint8)
    return (L[..., 0].copy(), R[..., 0].copy()) if c == 1 else (L.copy(), R.copy())


@functools.lru_cache(None)
def reference(w: int, h: int, c: int, shift: int, seed: int, items: tuple):
    """bm_numpy.bm of textured_pair(w, h, c, shift, seed) for Params(**dict(items)), computed once and shared (read-only)."""
    L, R = textured_pair(w, h, c, shift, seed)
    out = bn.bm(L, R, bn.Params(**dict(items)))
    out.setflags(write=False)
    return out
