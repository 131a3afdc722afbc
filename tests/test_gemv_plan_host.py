"""The decode GEMV dispatch without a GPU: teo_gemv_plan / teo_gemv_qkv_plan (csrc/gemv_plan.hip) against tests/golden/
gemv_dispatch_table.json -- the kernel instantiation and workgroup count the profiler's kernel trace reported for every call of
tools/gemv_dispatch_table.py's list, recorded from the library BEFORE the dispatch moved into the planner -- and the knob contract of
include/teo_hip.h read off the plans: a "bitwise" knob never changes the kernel form, nor U where U enters the fp32 order of the sums."""
import json
import os
import re

import pytest

from teochat_amd import _lib as L
from tests import _knobs
from tools import gemv_dispatch_table as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^(gemv_\w+) (\w+)/(\w+)/(\w+) R(\d+) U(\d+) pf([01]) x(\d) nt([01]) sw([01]) wg(\d+) lds(\d+) img(\d+)$")
BITWISE = [k for k in G.GEMV_KEYS if _knobs.KNOBS[k].contract == "bitwise"]


def plan(lib, c):
    """the plan line of one entry of the tool's list, under the bound tune block"""
    wfmt, dt = G.FORMATS[c["fmt"]]
    if c["kind"] == "qkv":
        return lib.teo_gemv_qkv_plan(c["K"], c["H"], c["Hk"], c["hd"], wfmt, dt).decode()
    return lib.teo_gemv_plan(c["N"], c["K"], wfmt, c["flags"], int(c["norm"]), dt, G.F32 if c["of32"] else dt).decode()


def fields(line):
    m = LINE.match(line)
    assert m, line
    kind, x, y, w = m.groups()[:4]
    R, U, pf, xpt, nt, sw, wg, lds, img = (int(v) for v in m.groups()[4:])
    return dict(kind=kind, x=x, y=y, w=w, R=R, U=U, pf=pf, xpt=xpt, nt=nt, sw=sw, wg=wg, lds=lds, img=img)


@pytest.fixture()
def tune():
    lib = L.load()
    t = L.Tune()
    t.bind()
    yield lib, t
    lib.teo_tune_bind(None)
    t.close()


def under(t, knobs):
    assert t.reset() == 0
    for k, v in knobs.items():
        assert t.set(k, v) == 0


def problems():
    """every distinct problem of the table's list (the entries without their knobs), in order"""
    seen, out = set(), []
    for c in G.flat(G.calls()):
        key = tuple(sorted((k, v) for k, v in c.items() if k != "knobs"))
        if key not in seen:
            seen.add(key)
            out.append({k: v for k, v in c.items() if k != "knobs"})
    return out


def test_gemv_plans_reproduce_the_recorded_kernel_trace(tune):
    """Every row of the table: the plan names the instantiation (kernel, types, R, U, prefetch, x chunks, nt, SwiGLU) and the workgroup count
    the trace of the parent library showed.  The dynamic LDS size is not in a trace (its LDS column is the static share): it is checked
    against what the kernels' layout needs -- the x image, padded to whole groups of 64 chunks, and 8 floats of scratch behind it."""
    lib, t = tune
    with open(os.path.join(ROOT, "tests", "golden", "gemv_dispatch_table.json")) as f:
        table = json.load(f)
    want = G.unrle(table["names"], table["runs"])
    entries = G.flat(G.calls())
    assert table["rows"] == len(want) == len(entries) and len(want) > 3000 and len(table["names"]) > 500
    assert {n.split()[0] for n in table["names"]} == {"gemv_rows", "gemv_splitk", "gemv_qkv_rope"}
    bad, knobs = [], None
    for c, w in zip(entries, want):
        if c["knobs"] is not knobs:
            knobs = c["knobs"]
            under(t, knobs)
        got = plan(lib, c)
        if got.rsplit(" lds", 1)[0] != w:
            bad.append((c, w, got))
            continue
        f = fields(got)
        ve = {"mxfp4": 32, "fp8": 16, "f32": 4}.get(f["w"], 8)
        need = 0 if f["kind"] == "gemv_splitk" else -(-(c["K"] // ve) // 64) * 64 * ve * (f["img"] // 8) + 32
        # the image's width is the kernels' own choice (gemv.hip BfImage / RowsImage16): 16 bits for one-byte weights, and for f16 in the row kernel
        img = 0 if f["kind"] == "gemv_splitk" else (16 if f["w"] in ("fp8", "mxfp4") or (f["w"] == "f16" and f["kind"] == "gemv_rows") else 32)
        if f["lds"] != need or f["img"] != img:
            bad.append((c, "lds %d img %d" % (need, img), got))
    assert not bad, (len(bad), bad[:10])


def test_bitwise_knobs_keep_the_kernel_form_and_the_order_of_the_sums(tune):
    """include/teo_hip.h calls gemv_nt, gemv_max_blocks, gemv_small_k, gemv_splitk_u and gemv_splitk_r bit-identical.  As data, for every
    problem of the table and every value tests/_knobs.py lists: the plan keeps the default plan's kernel; and where x is staged as a 16-bit
    image (one-byte weights; f16 in the row kernel), whose sums take U chunks at a time, it keeps U -- "the knob picks the prologue, not
    the order of the sums"."""
    lib, t = tune
    assert sorted(BITWISE) == ["gemv_max_blocks", "gemv_nt", "gemv_small_k", "gemv_splitk_r", "gemv_splitk_u"]
    probs = problems()
    assert len(probs) > 150
    under(t, {})
    base = [fields(plan(lib, c)) for c in probs]
    image16 = [b["img"] == 16 for b in base]
    assert sum(image16) > 40
    bad = []
    for key in BITWISE:
        for v in _knobs.values(key):
            under(t, {key: v})
            for c, b, i16 in zip(probs, base, image16):
                f = fields(plan(lib, c))
                if f["kind"] != b["kind"] or (i16 and f["U"] != b["U"]):
                    bad.append((key, v, c, b, f))
    assert not bad, (len(bad), bad[:5])


def test_a_w13_image_runs_the_geometry_of_the_bf16_matrix(tune):
    """tests/test_w13_gpu.py compares a w13 image bit for bit with the raw bf16 matrix under gemv_variant 0 / 1 / 2 and the bitwise knobs: that
    rests on both taking the same kernel form with the same R, U and x image (kind, R, U, img).  For every bf16 problem of the table:
    under gemv_variant 0 / 1 / 2, alone and crossed with every value of the bitwise knobs, the four are equal.  At the default gemv_variant
    they are equal too, with the one exception gemv_plan.hip states: the split-K form, where no (R, U) changes a bit (the chunk -> (wave,
    lane) map does not depend on them), caps its AUTOMATIC U at 2 for an image -- pinned here as exactly that."""
    lib, t = tune
    probs = [c for c in problems() if c["fmt"] == "bf16"]
    assert len(probs) > 25
    bitwise = [{k: v} for k in BITWISE for v in _knobs.values(k)]
    forced = [dict(b, gemv_variant=v) for v in (0, 1, 2) for b in [{}] + bitwise]
    bad, capped = [], 0
    for knobs in forced + [{}] + bitwise:
        under(t, knobs)
        for c in probs:
            a, b = fields(plan(lib, c)), fields(plan(lib, dict(c, fmt="w13")))
            assert b["w"] == "w13" and a["w"] == "bf16"
            same = all(a[k] == b[k] for k in ("kind", "R", "U", "img"))
            if not same and "gemv_variant" not in knobs and a["kind"] == "gemv_splitk" and not knobs.get("gemv_splitk_u"):
                capped += 1
                same = all(a[k] == b[k] for k in ("kind", "R", "img")) and a["U"] > 2 and b["U"] == 2
            if not same:
                bad.append((knobs, c, a, b))
    assert not bad and capped > 0, (len(bad), capped, bad[:5])


def test_a_refused_call_plans_to_nothing(tune):
    lib, _ = tune
    BF16, F16, F32 = G.BF16, G.F16, G.F32
    assert lib.teo_gemv_plan(512, 4096, G.NATIVE, 0, 1, BF16, BF16) != b""
    assert lib.teo_gemv_plan(512, 4100, G.NATIVE, 0, 1, BF16, BF16) == b"" and b"multiple of 8" in lib.teo_last_error()     # K not a multiple of the chunk
    assert lib.teo_gemv_plan(512, 4096 + 16, G.W4, 0, 1, BF16, BF16) == b""
    assert lib.teo_gemv_plan(512, 15360, G.NATIVE, 0, 1, BF16, BF16) == b"" and b"too large for LDS" in lib.teo_last_error()   # K above the LDS cap
    assert lib.teo_gemv_plan(512, 15344, G.NATIVE, 0, 1, BF16, BF16) != b""
    assert lib.teo_gemv_plan(512, 4096, G.W8, 0, 1, F16, F16) == b"" and b"fp8 weights need bf16" in lib.teo_last_error()      # fp8 with f16 activations
    assert lib.teo_gemv_plan(512, 4096, G.W13, 0, 1, F16, F16) == b""
    assert lib.teo_gemv_plan(512, 4096, G.NATIVE, 0, 1, F32, BF16) == b""                  # f32 inputs need an f32 output
    assert lib.teo_gemv_plan(500, 4096, G.NATIVE, G.SWIGLU, 1, BF16, BF16) == b""         # SwiGLU needs N % 32 == 0
    assert lib.teo_gemv_plan(512, 4096, 4, 0, 1, BF16, BF16) == b"" and lib.teo_gemv_plan(512, 4096, G.NATIVE, 0, 1, 7, BF16) == b""
    assert lib.teo_gemv_plan(0, 4096, G.NATIVE, 0, 1, BF16, BF16) == b""                   # N = 0 launches nothing
    assert lib.teo_gemv_qkv_plan(4096, 32, 32, 128, G.NATIVE, BF16) != b""
    assert lib.teo_gemv_qkv_plan(4096, 32, 32, 96, G.NATIVE, BF16) == b""                  # head_dim must be a power of two
    assert lib.teo_gemv_qkv_plan(4096 + 8, 32, 32, 128, G.W8, BF16) == b""
    assert lib.teo_gemv_qkv_plan(4096, 32, 32, 128, G.W4, F16) == b"" and lib.teo_gemv_qkv_plan(4096, 32, 32, 128, G.W13, F32) == b""
    assert lib.teo_gemv_qkv_plan(15360, 32, 32, 128, G.NATIVE, BF16) == b""
