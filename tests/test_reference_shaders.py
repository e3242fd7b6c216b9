"""The oracle held to the reference's own shader text, executed on the CPU.

oracle/ref_recipe.py turns shaders/{scale,motion,interpolate}.comp into C++ with five mechanical edits and compiles them
against oracle/glsl_shim.hpp (oracle/_ref/, never committed); oracle.ref_scale / ref_motion / ref_interpolate run them.  Every
exact GPU test of this suite compares a kernel with oracle/lfg_oracle.c, a hand restatement of those shaders: here that
restatement has to equal the executed text on every pixel -- a misread sign, loop bound, operator order or truncation shows --
with one exception that is asserted, not tolerated: interpolate.comp fetches its vector with texture(), the oracle with a plain
read (its choice (8)), and the two differ only at invocations whose texel centre fp32 misses (oracle.inexact_centres).

What is executed is the shader text.  What stays read: the built-in choices (1)-(7) and (9), which the shim takes from
lfg_oracle.c's header (tests/test_glsl_shim.py holds them to known answers), and the Vulkan host code.

The tests that run the shaders need the reference or an earlier oracle/_ref and skip, saying so, only without both; the tests
on tests/golden/ref_shaders.npz need neither.  CPU only."""
import hashlib
import importlib.util
import json
import os
import re
import time

import numpy as np
import pytest

import oracle
from linux_fg_amd import synth
from oracle import ref_recipe
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref():
    if not oracle.ref_available():
        pytest.skip(f"no reference shaders at {ref_recipe.reference_dir()} and no earlier build in oracle/_ref")
    return oracle


def first_bad(got, want):
    bad = np.argwhere((got != want).reshape(got.shape[0], got.shape[1], -1).any(-1))
    return f"{len(bad)} pixels differ, first (y, x) {bad[:3].tolist()}"


# ---- the recipe: nothing but the five edits stands between the .comp files and the compiler
#
# The five kinds, written a second time and without looking at the recipe's patterns: what each may turn a line into.

_LITERAL_F = re.compile(r"(?<![\w.])(\d+\.\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)f(?![\w.])")


def _allowed(kind, before):
    """What an edit of `kind` may make of the line `before`, or None where that kind does not apply to it."""
    if kind == "a":
        s = before.strip()
        return "" if s.startswith("#version") or (s.startswith("layout(local_size") and s.endswith(") in;")) else None
    if kind == "b":
        m = re.fullmatch(r"(\s*)layout\(binding = \d+(?:, \w+)?\) uniform (sampler2D|image2D) (\w+);", before)
        return f"{m.group(1)}{m.group(2)} {m.group(3)};" if m else None
    if kind == "c":
        old = "layout(push_constant) uniform PushConstants"
        return before.replace(old, "struct PushConstants") if old in before else None
    if kind == "d":
        return before.replace("void main()", "void shader_main()") if "void main()" in before else None
    raise AssertionError(f"unknown kind of edit {kind!r}")


def test_recipe_makes_the_five_edits_and_no_other(ref):
    if not ref_recipe.reference_present():
        pytest.skip(f"no reference shaders at {ref_recipe.reference_dir()} to compare oracle/_ref with")
    manifest = json.load(open(ref_recipe.MANIFEST_PATH))
    assert {"-O2", "-ffp-contract=off", "-fno-fast-math"} <= set(manifest["flags"])
    assert not {"-ffast-math", "-Ofast"} & set(manifest["flags"])
    assert set(manifest["shaders"]) == {"scale", "motion", "interpolate"}
    for name, entry in manifest["shaders"].items():
        raw = open(ref_recipe.shader_path(name), "rb").read()
        assert hashlib.sha256(raw).hexdigest() == entry["sha256"], name
        source = raw.decode().split("\n")
        generated = open(os.path.join(ref_recipe.REF_DIR, entry["generated"]), newline="").read().split("\n")
        first = entry["first_line"] - 1
        assert entry["lines"] == len(source)
        body = generated[first:first + len(source)]
        # around the body: includes, two defines, the namespace, the names -- and no line that could hold shader text
        around = generated[:first] + generated[first + len(source):]
        assert [line for line in around if line and not line.startswith(("//", "#include \"../", "#define LFG_REF_", "namespace lfg_ref_",
                                                                         "GLSL_SHIM_NAMES", "}  // namespace"))] == [], name
        kinds = {}
        for e in entry["edits"]:
            kinds.setdefault(e["line"], []).append(e["kind"])
        assert all(len(k) == len(set(k)) and set(k) <= set("abcde") for k in kinds.values())
        seen = set()
        for number, (before, after) in enumerate(zip(source, body), 1):
            if number not in kinds:
                assert after == before, f"{name}.comp:{number} changed without being listed"
                continue
            want = before
            for kind in [k for k in kinds[number] if k != "e"]:
                want = _allowed(kind, want)
                assert want is not None, f"{name}.comp:{number}: edit {kind} does not apply to {before!r}"
            if "e" in kinds[number]:
                # taking the suffixes off again gives the line as it was before (e), and at least one was put on
                assert _LITERAL_F.sub(r"\1", after) == want and after != want, f"{name}.comp:{number}: {before!r} -> {after!r}"
            else:
                assert after == want, f"{name}.comp:{number}: {before!r} -> {after!r}"
            seen |= set(kinds[number])
        assert seen == set("abcde"), (name, seen)
        # after (e) no floating literal is left a double, on any line
        code = "\n".join(line.partition("//")[0] for line in body)
        literals = list(re.finditer(r"(?<![\w.])(?:(?:\d+\.\d*|\.\d+)(?:[eE][-+]?\d+)?|\d+[eE][-+]?\d+)", code))
        assert literals and all(code[m.end():m.end() + 1] == "f" for m in literals), name


def test_ref_is_ignored_and_the_recipe_holds_no_shader_text():
    """oracle/_ref/ is ignored by git, and the committed parts of the recipe hold no shader text: none of the shaders' own
    function names occurs in them."""
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "oracle/_ref/" in ignore
    for name in ("glsl_shim.hpp", "ref_driver.inc", "ref_recipe.py"):
        text = open(os.path.join(ROOT, "oracle", name)).read()
        for word in ("sampleLanczos", "sampleWithMotion", "bestMotion", "totalWeight", "blockStart"):
            assert word not in text, (name, word)


# ---- scale.comp

SCALE_PAIRS = [((32, 18), (64, 36)),      # exact 2x
               ((20, 12), (33, 19)),      # ragged up
               ((20, 12), (13, 8)),       # down
               ((40, 30), (7, 3)),        # far down: taps skip texels
               ((17, 9), (17, 9)),        # identity
               ((1, 1), (5, 5)),          # one texel: most taps outside [0, 1]
               ((5, 3), (17, 4)),
               ((37, 23), (74, 46)),      # 2x of odd sizes
               ((30, 20), (45, 37))]      # larger than one 16 x 16 workgroup in both axes and no multiple of 16


@pytest.mark.parametrize("in_wh,out_wh", SCALE_PAIRS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scale_oracle_equals_the_executed_shader(ref, in_wh, out_wh):
    src = synth.noise_bytes(*in_wh, seed=100 * in_wh[0] + out_wh[0])
    got, want = oracle.scale(src, *out_wh), ref.ref_scale(src, *out_wh)
    assert (got == want).all(), first_bad(got, want)
    assert want.any()


# ---- motion.comp

MOTION_PARAMETERS = [(8, 16.0), (4, 3.0), (5, 2.0), (8, 0.0), (3, 2.5)]       # the last: a fractional radius


def motion_contents(w=40, h=30):
    prev = synth.make_prev(w, h, seed=5)
    pan = synth.translate(prev, (3, -2), seed=5).copy()
    pan[8:16, 20:30] = synth.noise_bytes(10, 8, 9)                            # matches broken by an occluder
    flat = np.empty((h, w, 4), np.uint8)
    flat[...] = (40, 90, 200, 255)                                             # every cost ties
    return {"pan": (prev, pan), "noise": (synth.noise_bytes(w, h, 1), synth.noise_bytes(w, h, 2)), "flat": (flat, flat)}


@pytest.mark.parametrize("content", ["pan", "noise", "flat"])
@pytest.mark.parametrize("bs,radius", MOTION_PARAMETERS)
def test_motion_oracle_equals_the_executed_shader(ref, content, bs, radius):
    """Whole frames of 40 x 30, so every border at which the block or the displaced block leaves the image is in them."""
    prev, curr = motion_contents()[content]
    xy, zw = ref.ref_motion(prev, curr, bs, radius, with_zw=True)
    got = oracle.motion(prev, curr, bs, radius)
    assert (got == xy).all(), first_bad(got, xy)
    assert (zw[..., 0] == 0).all() and (zw[..., 1] == 1).all()                # the stored texel is (best, 0, 1)
    if content != "flat" and radius >= 2:
        assert len(np.unique(xy.reshape(-1, 2), axis=0)) > 3                   # the case tells vectors apart
    if radius == 2.5:
        assert set(np.unique(xy)) <= {-2.5, -1.5, -0.5, 0.0, 0.5, 1.5, 2.5}    # (0 is the initial bestMotion)


def test_motion_on_a_region_of_a_larger_frame(ref):
    """128 x 72 at radius 16 through the region argument: an aligned region at the bottom-right corner and a ragged one in the
    interior, which runs as whole workgroups and stores its own pixels only."""
    prev, curr = synth.make_pair(128, 72, stream=2, shift=(-4, 3))
    for roi in ((112, 56, 128, 72), (37, 21, 50, 30)):
        x0, y0, x1, y1 = roi
        got, want = oracle.motion(prev, curr, roi=roi), ref.ref_motion(prev, curr, roi=roi)
        assert (got == want).all(), (roi, first_bad(got, want))
        outside = np.ones((72, 128), bool)
        outside[y0:y1, x0:x1] = False
        assert (want[outside] == 0).all() and (want[y0:y1, x0:x1] != 0).any()


# ---- interpolate.comp
#
# On cases.sampling_scene: independent noise frames and per-pixel vectors in every row and column.

INTERPOLATE_FACTORS = (0.25, 0.5, 0.3, 0.9)
EXACT_SIZES = [(64, 32), (30, 18), (48, 20)]         # every texel centre is exact in fp32
INEXACT_SIZES = [(100, 36), (200, 120), (33, 90)]
INEXACT_TABLE = {64: 0, 90: 10, 100: 8, 120: 3, 200: 16, 1080: 42, 1920: 51, 2160: 85, 3840: 102}


def formula_mask(w, h):
    return oracle.inexact_centres(w)[None, :] | oracle.inexact_centres(h)[:, None]


def test_inexact_centres_are_counted():
    """How many indices of 0 .. n-1 miss their own texel centre in fp32, at the sizes of the tests and of real frames.  The
    formula is written out here a second time, in float64 with explicit roundings."""
    assert {n: int(oracle.inexact_centres(n).sum()) for n in INEXACT_TABLE} == INEXACT_TABLE
    fl = lambda v: np.float32(v).astype(np.float64)  # noqa: E731
    for n in (90, 100, 1080):
        i = np.arange(n, dtype=np.float64)
        slow = fl(fl(fl((i + 0.5) / n) * n) - 0.5) != i
        assert (slow == oracle.inexact_centres(n)).all()


@pytest.mark.parametrize("wh", EXACT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_interpolate_oracle_equals_the_executed_shader_where_centres_are_exact(ref, wh):
    prev, curr, mv = cases.sampling_scene_of(*wh)
    assert not formula_mask(*wh).any()
    for t in INTERPOLATE_FACTORS:
        want, mask = ref.ref_interpolate(prev, curr, mv.astype(np.float32), t)
        assert not mask.any(), (t, int(mask.sum()))
        got = oracle.interpolate(prev, curr, mv.astype(np.float32), t)
        assert (got == want).all(), (t, first_bad(got, want))


@pytest.mark.parametrize("wh", INEXACT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_interpolate_oracle_differs_from_the_executed_shader_only_where_a_centre_is_missed(ref, wh):
    """Choice (8) of lfg_oracle.c, bounded: outside the mask the oracle is the shader; the mask is the columns and rows of the
    formula and no more than 12 % of the image; and inside it some pixel does differ, so the finding stays in sight and the
    mask cannot become a place to hide."""
    prev, curr, mv = cases.sampling_scene_of(*wh)
    for t in INTERPOLATE_FACTORS:
        want, mask = ref.ref_interpolate(prev, curr, mv.astype(np.float32), t)
        got = oracle.interpolate(prev, curr, mv.astype(np.float32), t)
        differ = (got != want).any(-1)
        levels = int(np.abs(got.astype(np.int16) - want.astype(np.int16)).max())
        print(f"{wh[0]}x{wh[1]} t={t}: mask {mask.mean():.1%}, {int(differ.sum())} pixels differ inside it by up to {levels} levels")
        assert (mask == formula_mask(*wh)).all()
        assert mask.mean() <= 0.12
        assert not (differ & ~mask).any(), (t, first_bad(np.where(mask[..., None], want, got), want))
        assert (differ & mask).any(), t


# ---- the committed fixtures

def test_golden_small_equals_a_fresh_run_of_the_shaders(ref):
    """tests/golden/golden_small.npz was written by the oracle; every output in it is also what the executed shaders give for
    its inputs, so the GPU tests that read it are held to the shaders."""
    g = np.load(os.path.join(GOLDEN, "golden_small.npz"))
    started = time.time()
    assert (ref.ref_scale(g["prev_in"], 128, 72) == g["prev_up"]).all()
    assert (ref.ref_scale(g["curr_in"], 128, 72) == g["curr_up"]).all()
    assert (ref.ref_scale(g["curr_in"], 53, 41) == g["curr_53x41"]).all()
    assert (ref.ref_motion(g["prev_up"], g["curr_up"], 8, 16.0) == g["mv"]).all()
    assert (ref.ref_motion(g["prev_in"], g["curr_in"], 4, 3.0) == g["mv_b4_r3"]).all()
    for name, t in (("interp_25", 0.25), ("interp_50", 0.5), ("interp_75", 0.75)):
        frame, mask = ref.ref_interpolate(g["prev_up"], g["curr_up"], g["mv"].astype(np.float32), t)
        assert not mask.any() and (frame == g[name]).all(), name
    assert set(g.files) == {"prev_in", "curr_in", "prev_up", "curr_up", "curr_53x41", "mv", "mv_b4_r3", "interp_25", "interp_50", "interp_75"}
    print(f"golden_small.npz: 8 outputs equal the executed shaders ({time.time() - started:.1f} s)")


def load_ref_golden():
    return np.load(os.path.join(GOLDEN, "ref_shaders.npz"))


def test_ref_shaders_fixture_equals_a_fresh_run(ref):
    spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(GOLDEN, "make_ref_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    fresh, g = module.build(), load_ref_golden()
    assert set(fresh) == set(g.files)
    for name, value in fresh.items():
        assert value.dtype == g[name].dtype and value.shape == g[name].shape and (value == g[name]).all(), name


def test_ref_shaders_fixture_is_small_and_holds_what_it_says():
    g = load_ref_golden()
    size = os.path.getsize(os.path.join(GOLDEN, "ref_shaders.npz"))
    assert size <= os.path.getsize(os.path.join(GOLDEN, "golden_small.npz")) and size <= 96 * 1024
    assert (g["mask_100"] == formula_mask(100, 36)).all() and g["mask_100"].any() and g["mask_100"].mean() <= 0.12
    for w in (64, 100):
        mv = g[f"mv_{w}_b8_r16"]
        assert len(np.unique(mv.reshape(-1, 2), axis=0)) > 8 and (mv == 0).all(-1).mean() > 0.5
        assert g[f"interp_{w}_50"].any(-1).mean() > 0.5      # most of the frame is sampled, not black


def test_oracle_equals_the_ref_shaders_fixture():
    """Needs no reference: the oracle against what the executed shaders gave when the fixture was written -- exactly, and
    outside the mask where there is one; inside it the fixture keeps at least one pixel on which the two part."""
    g = load_ref_golden()
    assert (oracle.scale(g["scale_in"], 13, 8) == g["scale_13x8"]).all()
    assert (oracle.scale(g["scale_in"], 33, 19) == g["scale_33x19"]).all()
    assert (oracle.motion(g["prev_100"], g["curr_100"], 4, 3.0) == g["mv_100_b4_r3"]).all()
    parted = 0
    for w in (64, 100):
        prev, curr, mv = g[f"prev_{w}"], g[f"curr_{w}"], g[f"mv_{w}_b8_r16"]
        assert (oracle.motion(prev, curr, 8, 16.0) == mv).all()
        mask = g["mask_100"] if w == 100 else np.zeros(mv.shape[:2], bool)
        for t in (50, 30):
            got, want = oracle.interpolate(prev, curr, mv.astype(np.float32), t / 100), g[f"interp_{w}_{t}"]
            differ = (got != want).any(-1)
            assert not (differ & ~mask).any(), (w, t, first_bad(np.where(mask[..., None], want, got), want))
            parted += int(differ.sum())
    assert parted > 0
