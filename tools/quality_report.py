"""How close each route's generated frame comes to a frame that was held out, measured on the GPU: the table of DESIGN.md
section 4.11 at 1080p and 4K.  The pair is frames 0 and 2 of a synth triple, frame 1 is the truth, the factor 0.5; PSNR and
differing pixels are taken over R, G and B (mask 0x7).  Three triples: a pan of (3, -2) per frame; a pan of (20, -12) per
frame, whose pair's (40, -24) is beyond the full search's 16 px and inside the pyramid's reach; the first pan with +-4 levels
of independent noise on all three frames; the first pan under a HUD of thin white glyphs and bars that stands still in all three
frames.  Seven routes: repeating frame 0, and lfg_interpolate_frames under six settings, the last with
static-overlay protection (lfg_set_static_protection at tolerance 0).
Beside PSNR each route gets its SSIM over the same channels (lfg_frame_ssim: the mean over the 8 x 8 windows) and the number of
windows below 0.5, which a halo or a torn overlay moves and a uniform error of the same size does not.
Everything goes through lfg_interpolate_frames + lfg_frame_diff + lfg_frame_ssim, with one sync per route (the read of its records).

    python tools/quality_report.py [--sizes 1080p,4k] [--json out.json] [--out report.txt]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys

import numpy as np

from stage_bench import SIZES, emit, write_json                # (puts the repository root on sys.path)
from linux_fg_amd import capi, synth  # noqa: E402

MASK = 0x7
ROUTES = [                                     # (name, estimator, refinement radius, interpolator, semantics[, static tolerance])
    ("full search, shader, reference semantics (the default)", capi.ESTIMATOR_FULL_SEARCH, -1, capi.INTERPOLATOR_SHADER, capi.SEMANTICS_REFERENCE),
    ("full search, shader, intended semantics", capi.ESTIMATOR_FULL_SEARCH, -1, capi.INTERPOLATOR_SHADER, capi.SEMANTICS_INTENDED),
    ("full search, compensated", capi.ESTIMATOR_FULL_SEARCH, -1, capi.INTERPOLATOR_COMPENSATED, capi.SEMANTICS_INTENDED),
    ("full search, refine radius 1, compensated", capi.ESTIMATOR_FULL_SEARCH, 1, capi.INTERPOLATOR_COMPENSATED, capi.SEMANTICS_INTENDED),
    ("pyramid, compensated", capi.ESTIMATOR_PYRAMID, -1, capi.INTERPOLATOR_COMPENSATED, capi.SEMANTICS_INTENDED),
    ("full search, compensated, static protection 0", capi.ESTIMATOR_FULL_SEARCH, -1, capi.INTERPOLATOR_COMPENSATED, capi.SEMANTICS_INTENDED, 0),
]


def glyphs(w, h):
    """(H, W) bool: the glyph overlay of DESIGN.md section 4.13 -- eight 6 x 9 glyphs of 1 px strokes, a 1 px bar and a 2 px
    bar per 200 x 120 tile -- repeated over the frame."""
    tile = np.zeros((120, 200), bool)
    for k in range(8):
        x = 20 + 10 * k
        tile[12:21, x] = True
        for r in (12, 16, 20):
            tile[r, x:x + 6] = True
    tile[100, 10:190] = True
    tile[96:112, 150:152] = True
    return np.tile(tile, (-(-h // 120), -(-w // 200)))[:h, :w]


def triples(w, h):
    """(name, frame 0, frame 1, frame 2)"""
    for name, shift in (("pan(3,-2)", (3, -2)), ("pan(20,-12)", (20, -12))):
        f0 = synth.make_prev(w, h)
        f1 = synth.translate(f0, shift)
        yield name, f0, f1, synth.translate(f1, shift)
    f0 = synth.make_prev(w, h)
    f1 = synth.translate(f0, (3, -2))
    clean = [f0, f1, synth.translate(f1, (3, -2))]
    rng = np.random.default_rng(11)
    yield ("pan(3,-2)+-4noise", *[np.clip(f.astype(np.int16) + rng.integers(-4, 5, f.shape), 0, 255).astype(np.uint8) for f in clean])
    hud = [f.copy() for f in clean]
    for f in hud:
        f[glyphs(w, h)] = 255
    yield ("pan(3,-2)+glyphs", *hud)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,4k")
    ap.add_argument("--json", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    with capi.Context(0) as ctx:
        for size in a.sizes.split(","):
            w, h = SIZES[size]
            for content, f0, f1, f2 in triples(w, h):
                p, t, c, o = ctx.frame_from(f0), ctx.frame_from(f1), ctx.frame_from(f2), ctx.create_frame(w, h)
                r, rs = ctx.create_diff_record(), ctx.create_ssim_record()

                def row(route):
                    s = capi.summarize(ctx.read_diff_record(r), MASK)       # the route's one sync
                    q = capi.summarize_ssim(ctx.read_ssim_record(rs), MASK)
                    emit(rows, {"size": size, "content": content, "route": route, "psnr_db": s["psnr_db"], "differing": s["differing"],
                                "over_1": s["over_1"], "p50": s["p50"], "p99": s["p99"], "max_abs": s["max_abs"], "pixels": s["pixels"],
                                "ssim": q["all"], "below_half": q["below_half"], "worst_ssim": q["worst_value"], "windows": q["windows"]})

                ctx.frame_diff(p, t, r, MASK)
                ctx.frame_ssim(p, t, rs, MASK)
                row("repeat prev (no generation)")
                for name, estimator, radius, interpolator, semantics, *tolerance in ROUTES:
                    ctx.set_static_protection(tolerance[0] if tolerance else -1)
                    ctx.set_motion_estimator(estimator)
                    ctx.set_vector_refinement(radius)
                    ctx.set_interpolator(interpolator)
                    ctx.set_semantics(semantics)
                    ctx.interpolate_frames(p, c, o, 0.5)
                    ctx.frame_diff(o, t, r, MASK)
                    ctx.frame_ssim(o, t, rs, MASK)
                    row(name)
                for f in (p, t, c, o, r, rs):
                    ctx.destroy_frame(f)
    write_json(a.json, rows)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"# lib_sha16 {hashlib.sha256(open(capi.LIB_PATH, 'rb').read()).hexdigest()[:16]}\n")
            f.write(f"# python tools/quality_report.py {' '.join(sys.argv[1:])}: frames 0 and 2 of a synth triple generate frame 1 at 0.5;\n"
                    "# lfg_interpolate_frames + lfg_frame_diff + lfg_frame_ssim on one MI355X; PSNR, differing pixels, SSIM and the windows\n"
                    "# below 0.5 over R, G and B (mask 0x7).\n")
            for row_ in rows:
                f.write(json.dumps(row_) + "\n")
            for size in a.sizes.split(","):
                f.write(f"\n## {size}: PSNR dB / differing px of {SIZES[size][0] * SIZES[size][1]:,} / SSIM / windows below 0.5\n")
                names = list(dict.fromkeys(x["content"] for x in rows))
                f.write("| route | " + " | ".join(names) + " |\n|---|" + "---|" * len(names) + "\n")
                for route in dict.fromkeys(x["route"] for x in rows):
                    cells = [next(x for x in rows if (x["size"], x["content"], x["route"]) == (size, n, route)) for n in names]
                    f.write(f"| {route} | " + " | ".join(f"{x['psnr_db']:.2f} / {x['differing']:,} / {x['ssim']:.4f} / {x['below_half']:,}" for x in cells) + " |\n")


if __name__ == "__main__":
    main()
