#!/usr/bin/env python3
"""Generates tests/golden/ref_shaders.npz: inputs, and what the reference's own shaders gave for them when their text ran on
the CPU (oracle/ref_recipe.py, oracle.ref_scale / ref_motion / ref_interpolate).  Data only.  It holds what golden_small.npz
lacks: a downscale and a ragged upscale; motion at (blockSize, searchRadius) = (4, 3) and (8, 16) on pairs with a flat patch
(every candidate ties) and an occluder of fresh noise (no candidate matches); interpolate on those pairs' own (8, 16) vectors
at 64x32, where every texel centre is exact in fp32, and at 100x36, where eight columns are not -- with the mask of the
invocations whose vector fetch had a non-zero fractional weight, the only place the oracle (choice (8) of lfg_oracle.c) and the
kernels may differ from the shader.

The backgrounds are static: under the shaders' literal semantics a pixel-unit vector is added to normalised uv, so a pixel
whose vector is not (0, 0) samples outside [0, 1] and comes out black, and a panned pair would be a black frame.

tests/test_reference_shaders.py holds this file to a fresh run of the shaders, so it cannot go stale, and holds the oracle to
it; tests/test_gpu_reference_shaders.py holds the kernels to it.  Needs the reference (or an earlier oracle/_ref):

    python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from linux_fg_amd import synth  # noqa: E402

FACTORS = (0.5, 0.3)


def pair(w, h, seed):
    """A static textured background; a flat patch in both frames; a square that moved by (3, -1); an occluder of fresh noise
    in curr only."""
    prev = synth.make_prev(w, h, seed=seed)
    curr = prev.copy()
    for f in (prev, curr):
        f[h // 2:h // 2 + 10, 4:18] = (90, 140, 200, 255)
    x = 4 * w // 5
    curr[4:12, x:x + 9] = prev[5:13, x - 3:x + 6]
    # At w = 100 the occluder's non-zero vectors end in column 57, and column 58's centre falls short of itself in fp32: its
    # bilinear vector fetch takes a little of column 57's vector, which is where the shader and choice (8) part.
    x = 46 * w // 100
    curr[h // 3:h // 3 + 12, x:x + 14] = synth.noise_bytes(14, 12, seed + 1)
    return prev, curr


def build():
    out = {}
    src = synth.noise_bytes(20, 12, 2012)
    out["scale_in"] = src
    out["scale_13x8"] = oracle.ref_scale(src, 13, 8)
    out["scale_33x19"] = oracle.ref_scale(src, 33, 19)
    for w, h in ((64, 32), (100, 36)):
        prev, curr = pair(w, h, 1000 * w + h)
        mv = oracle.ref_motion(prev, curr, 8, 16.0)
        assert (mv == mv.astype(np.int8)).all()
        out[f"prev_{w}"], out[f"curr_{w}"], out[f"mv_{w}_b8_r16"] = prev, curr, mv.astype(np.int8)
        for t in FACTORS:
            frame, mask = oracle.ref_interpolate(prev, curr, mv, t)
            out[f"interp_{w}_{int(t * 100)}"] = frame
            if w == 100:
                out.setdefault("mask_100", mask)
                assert (mask == out["mask_100"]).all()
            else:
                assert not mask.any()
    out["mv_100_b4_r3"] = oracle.ref_motion(out["prev_100"], out["curr_100"], 4, 3.0).astype(np.int8)
    return out


if __name__ == "__main__":
    out = build()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_shaders.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})
