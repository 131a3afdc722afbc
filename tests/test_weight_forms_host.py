"""The one weight-format check of the C ABI (llama_weights_check, teochat_amd/csrc/abi.hip), host side: a table of descriptor variants
against every entry point that takes a LLaMA descriptor and reads its layer weights.  Nothing is launched and no GPU is needed: argument
checks return before any HIP call, and a variant a use accepts is handed a workspace of 0 bytes, which every entry refuses
(TEO_ERR_WORKSPACE) before its first launch.

The expected codes are those of the three checks this one replaced (the prefill check, the weight half of the batched state check, the
block at the top of the single-conversation step), row for row, with three differences:
  1. a descriptor with no 16-bit layer arrays and no fp8 / MXFP4 copies is TEO_ERR_ARG at the single step too (the row "no weights at
     all"); before, the step passed it and read a null host pointer;
  2. the graph-create entries reject a bad descriptor before they touch the stream (before: inside the capture), so here they get
     rejected variants only, with a dummy stream handle;
  3. the profiled single step rejects it before its first recorded event (before: after).  Every profiled entry gets rejected variants
     only: with an accepted one it enqueues its hold kernel in front of the step, whose workspace check comes too late to stop a launch.
teo_llama_decode_begin reads no layer weights and checks none: every variant reaches its workspace check.  teo_kv_fork and the
*_workspace_bytes / *_workspace_status entries take a descriptor but no weights, and are not called here."""
import ctypes as C

import pytest

from teochat_amd import _lib as L

ARG, UNS, WS = -1, -2, -4             # TEO_ERR_ARG, TEO_ERR_UNSUPPORTED, TEO_ERR_WORKSPACE (= the use accepts the variant)
KINDS = ("qkv", "o", "gateup", "down")
EIGHT = tuple(k + s for k in KINDS for s in ("_w4", "_e4"))
FAKE = 0x10000                        # a non-null "device" address: compared with NULL on the host, never read
LAYERS, HEADS, HEAD_DIM, VOCAB, MAX_SEQ = 1, 1, 128, 32, 64


def variant(dtype=L.TEO_BF16, hidden=128, inter=128, w16=True, w8=False, head8=False, w4=(), p13=False, head13=False, prefill_w4=0,
            prefill_w4a8=0, prefill_fp8=0):
    """w4: the names among EIGHT that are set"""
    return dict(dtype=dtype, hidden=hidden, inter=inter, w16=w16, w8=w8, head8=head8, w4=tuple(w4), p13=p13, head13=head13,
                prefill_w4=prefill_w4, prefill_w4a8=prefill_w4a8, prefill_fp8=prefill_fp8)


def _rows():
    """(name, variant, (prefill, single step, batched step with w_mxfp4 = 0, batched step with w_mxfp4 = 1 and w_tiled = 1))"""
    rows = []
    for tag, dt in (("", L.TEO_BF16), (" f16", L.TEO_F16)):
        f16 = dt == L.TEO_F16
        v = lambda **kw: variant(dtype=dt, **kw)      # noqa: E731
        rows += [
            ("16-bit only" + tag, v(), (WS, WS, WS, ARG)),
            ("+_w8" + tag, v(w8=True, head8=True), (WS, WS, WS, ARG)),
            ("+_w4/_e4 complete" + tag, v(w4=EIGHT), (WS, ARG if f16 else WS, WS, ARG if f16 else WS)),
            ("+_w4/_e4 complete, prefill_w4" + tag, v(w4=EIGHT, prefill_w4=1), (ARG if f16 else WS, ARG if f16 else WS, WS, ARG if f16 else WS)),
            ("_w4 beside _w8" + tag, v(w8=True, w4=EIGHT), (WS, ARG, WS, ARG)),
            ("_w4 beside _w8, prefill_w4" + tag, v(w8=True, w4=EIGHT, prefill_w4=1), (ARG, ARG, WS, ARG)),
            ("_w4 with lm_head8" + tag, v(head8=True, w4=EIGHT), (WS, ARG, WS, ARG)),
            ("_w4 with lm_head8, prefill_w4" + tag, v(head8=True, w4=EIGHT, prefill_w4=1), (ARG, ARG, WS, ARG)),
            ("_p13 alone" + tag, v(p13=True, head13=True), (WS, ARG if f16 else WS, WS, ARG)),
            ("lm_head_p13 alone" + tag, v(head13=True), (WS, ARG if f16 else WS, WS, ARG)),
            ("_p13 beside _w8" + tag, v(p13=True, w8=True, head8=True), (WS, ARG, WS, ARG)),
            ("lm_head_p13 beside lm_head8" + tag, v(head13=True, head8=True), (WS, ARG, WS, ARG)),
            ("_p13 beside _w4" + tag, v(p13=True, w4=EIGHT), (WS, ARG, WS, ARG if f16 else WS)),
        ]
        for gone in EIGHT:
            some = tuple(n for n in EIGHT if n != gone)
            rows.append((f"{gone} missing{tag}", v(w4=some), (WS, ARG, WS, ARG)))
            rows.append((f"{gone} missing, prefill_w4{tag}", v(w4=some, prefill_w4=1), (ARG, ARG, WS, ARG)))
    rows += [
        # hidden 136: a multiple of 8 (the w13 rule) and not of 128 (the MXFP4 GEMMs' rule, which the single step's GEMV does not have)
        ("hidden 136, 16-bit only", variant(hidden=136), (WS, WS, WS, ARG)),
        ("hidden 136, _p13", variant(hidden=136, p13=True, head13=True), (WS, WS, WS, ARG)),
        ("hidden 136, _w4/_e4 complete", variant(hidden=136, w4=EIGHT), (WS, WS, WS, UNS)),
        ("hidden 136, _w4/_e4 complete, prefill_w4", variant(hidden=136, w4=EIGHT, prefill_w4=1), (UNS, WS, WS, UNS)),
        ("inter 136, _w4/_e4 complete, prefill_w4", variant(inter=136, w4=EIGHT, prefill_w4=1), (UNS, WS, WS, UNS)),
        ("hidden 132, _p13", variant(hidden=132, p13=True), (WS, ARG, WS, ARG)),
        ("inter 132, _p13", variant(inter=132, p13=True), (WS, ARG, WS, ARG)),
        # a 4-bit-only descriptor: NULL 16-bit layer arrays
        ("4-bit only", variant(w16=False, w4=EIGHT), (ARG, WS, ARG, WS)),
        ("4-bit only, prefill_w4", variant(w16=False, w4=EIGHT, prefill_w4=1), (WS, WS, ARG, WS)),
        ("4-bit only, prefill_w4 + prefill_w4a8", variant(w16=False, w4=EIGHT, prefill_w4=1, prefill_w4a8=1), (WS, WS, ARG, WS)),
        ("fp8 copies and no 16-bit arrays", variant(w16=False, w8=True, head8=True), (ARG, WS, WS, ARG)),
        ("prefill_w4a8 without prefill_w4", variant(w4=EIGHT, prefill_w4a8=1), (ARG, WS, WS, WS)),
        ("prefill_w4 with prefill_fp8", variant(w4=EIGHT, prefill_w4=1, prefill_fp8=1), (ARG, WS, WS, WS)),
        ("prefill_w4 without the arrays", variant(prefill_w4=1), (ARG, WS, WS, ARG)),
        ("prefill_w4a8 over inter 12416", variant(inter=12416, w4=EIGHT, prefill_w4=1, prefill_w4a8=1), (UNS, WS, WS, WS)),
        ("no weights at all", variant(w16=False), (ARG, ARG, ARG, ARG)),
    ]
    return rows


ROWS = _rows()


class Desc:
    """an L.LlamaDesc of tiny dimensions over host-valid pointer arrays of dummy addresses, kept alive beside it"""

    def __init__(self, v):
        self.keep = [L.Tune()]
        d = L.LlamaDesc()
        d.hidden, d.heads, d.kv_heads, d.head_dim, d.inter, d.layers, d.vocab = v["hidden"], HEADS, HEADS, HEAD_DIM, v["inter"], LAYERS, VOCAB
        d.eps, d.dtype, d.max_seq, d.max_pos = 1e-5, v["dtype"], MAX_SEQ, MAX_SEQ
        d.embed = d.final_norm_w = d.lm_head = d.rope_cos = d.rope_sin = FAKE
        names = ["in_norm_w", "post_norm_w", "k_cache", "v_cache", "vt_cache"]
        names += [k + "_w" for k in KINDS] if v["w16"] else []
        names += [k + s for k in KINDS for s in ("_w8", "_s")] if v["w8"] else []
        names += list(v["w4"])
        names += [k + "_p13" for k in KINDS] if v["p13"] else []
        for n in names:
            arr, pp = L.ptr_array([FAKE] * LAYERS)
            self.keep.append(arr)
            setattr(d, n, pp)
        if v["head8"]:
            d.lm_head8 = d.lm_head_s = FAKE
        if v["head13"]:
            d.lm_head_p13 = FAKE
        d.prefill_w4, d.prefill_w4a8, d.prefill_fp8 = v["prefill_w4"], v["prefill_w4a8"], v["prefill_fp8"]
        d.tune = self.keep[0].ptr
        self.d = d


def _loop_state(s):
    for f in ("d_token", "d_pos", "d_out_tokens", "d_out_count", "d_stop", "d_stop_ids", "d_logits", "d_rng"):
        setattr(s, f, FAKE)
    s.n_stop_ids, s.do_sample, s.top_k, s.temperature, s.top_p = 0, 0, 0, 1.0, 1.0
    return s


def _batch_state(cls, w4):
    s = _loop_state(cls())
    s.batch, s.out_stride, s.cache_stride, s.w_tiled, s.gateup_block8, s.w_mxfp4 = 2, 8, HEADS * MAX_SEQ * HEAD_DIM, w4, 0, w4
    if cls is L.DecodeStreamState:
        s.d_limit = FAKE
    return s


def _verify_state(w4):
    s = _loop_state(L.VerifyState())
    s.rows, s.max_new, s.ngram_max, s.w_tiled, s.gateup_block8, s.w_mxfp4 = 2, 4, 2, w4, 0, w4
    s.d_rows = s.d_n_draft = s.d_hist = s.d_hist_len = s.d_stats = FAKE
    return s


def entries(lib, d, use):
    """[(entry name, call() -> status, takes accepted variants too)] of one use: "prefill", "step", "batch" (w_mxfp4 = 0) or "batch4".
    Workspace: a non-null pointer with 0 bytes.  Plain steps go to the null stream; the graph-create entries need a stream handle and get
    a dummy one."""
    p, ws, stream, S = C.byref(d), FAKE, FAKE, 4
    if use == "prefill":
        lens, slots, pasts = (C.c_int * 2)(2, 2), (C.c_int * 2)(1, 0), (C.c_int * 2)(0, 0)
        stride = HEADS * MAX_SEQ * HEAD_DIM
        return [
            ("teo_llama_prefill", lambda: lib.teo_llama_prefill(p, FAKE, FAKE, S, 0, 1, FAKE, ws, 0, None, None), True),
            ("teo_llama_prefill_attentions", lambda: lib.teo_llama_prefill_attentions(p, FAKE, FAKE, S, 0, 1, FAKE, ws, 0, None, None, FAKE), True),
            ("teo_llama_prefill_batch", lambda: lib.teo_llama_prefill_batch(p, FAKE, lens, 2, stride, 1, FAKE, ws, 0, None, None), True),
            ("teo_llama_prefill_slots", lambda: lib.teo_llama_prefill_slots(p, FAKE, lens, slots, 2, stride, 1, FAKE, ws, 0, None, None), True),
            ("teo_llama_prefill_slots_past", lambda: lib.teo_llama_prefill_slots_past(p, FAKE, lens, pasts, slots, 2, stride, 1, FAKE, ws, 0, None, None), True),
            ("teo_llama_prefill_branches", lambda: lib.teo_llama_prefill_branches(p, FAKE, FAKE, FAKE, S, 0, FAKE, ws, 0, None), True),
        ]
    g = L.Guide()
    g.d_next, g.n_states, g.vocab, g.d_state, g.fallback_token = FAKE, 2, VOCAB, FAKE, 0
    sh = L.Share()
    sh.d_lead = sh.d_rows = FAKE
    ms, ct, out = (C.c_float * 8)(), (C.c_int * 8)(), C.c_void_p()
    if use == "step":
        s = C.byref(_loop_state(L.DecodeState()))
        return [
            ("teo_llama_decode_step", lambda: lib.teo_llama_decode_step(p, s, ws, 0, None), True),
            ("teo_llama_decode_step_guided", lambda: lib.teo_llama_decode_step_guided(p, s, C.byref(g), ws, 0, None), True),
            ("teo_llama_decode_step_profile", lambda: lib.teo_llama_decode_step_profile(p, s, ws, 0, ms, ct, None), False),
            ("teo_llama_decode_graph_create", lambda: lib.teo_llama_decode_graph_create(p, s, ws, 0, stream, C.byref(out)), False),
            ("teo_llama_decode_graph_create_guided", lambda: lib.teo_llama_decode_graph_create_guided(p, s, C.byref(g), ws, 0, stream, C.byref(out)), False),
        ]
    w4 = 1 if use == "batch4" else 0
    b, t, v = C.byref(_batch_state(L.DecodeBatchState, w4)), C.byref(_batch_state(L.DecodeStreamState, w4)), C.byref(_verify_state(w4))
    return [
        ("teo_llama_decode_batch_begin", lambda: lib.teo_llama_decode_batch_begin(p, b, ws, 0, None), True),
        ("teo_llama_decode_batch_step", lambda: lib.teo_llama_decode_batch_step(p, b, ws, 0, None), True),
        ("teo_llama_decode_batch_step_profile", lambda: lib.teo_llama_decode_batch_step_profile(p, b, ws, 0, ms, ct, None), False),
        ("teo_llama_decode_batch_graph_create", lambda: lib.teo_llama_decode_batch_graph_create(p, b, ws, 0, stream, C.byref(out)), False),
        ("teo_llama_decode_stream_step", lambda: lib.teo_llama_decode_stream_step(p, t, ws, 0, None), True),
        ("teo_llama_decode_stream_arm", lambda: lib.teo_llama_decode_stream_arm(p, t, 1, ws, 0, None), True),
        ("teo_llama_decode_stream_step_guided", lambda: lib.teo_llama_decode_stream_step_guided(p, t, C.byref(g), ws, 0, None), True),
        ("teo_llama_decode_stream_step_shared", lambda: lib.teo_llama_decode_stream_step_shared(p, t, C.byref(sh), None, ws, 0, None), True),
        ("teo_llama_decode_stream_graph_create", lambda: lib.teo_llama_decode_stream_graph_create(p, t, ws, 0, stream, C.byref(out)), False),
        ("teo_llama_decode_stream_graph_create_guided",
         lambda: lib.teo_llama_decode_stream_graph_create_guided(p, t, C.byref(g), ws, 0, stream, C.byref(out)), False),
        ("teo_llama_decode_stream_graph_create_shared",
         lambda: lib.teo_llama_decode_stream_graph_create_shared(p, t, C.byref(sh), C.byref(g), ws, 0, stream, C.byref(out)), False),
        ("teo_llama_verify_begin", lambda: lib.teo_llama_verify_begin(p, v, ws, 0, None), True),
        ("teo_llama_verify_step", lambda: lib.teo_llama_verify_step(p, v, ws, 0, None), True),
        ("teo_llama_verify_step_profile", lambda: lib.teo_llama_verify_step_profile(p, v, ws, 0, ms, ct, None), False),
        ("teo_llama_verify_graph_create", lambda: lib.teo_llama_verify_graph_create(p, v, ws, 0, stream, C.byref(out)), False),
    ]


USES = ("prefill", "step", "batch", "batch4")


def status_table(lib, name, v, want, skip=lambda entry: False):
    """{(use, entry): (status, expected)} of one row over every entry it may be given to"""
    got = {}
    desc = Desc(v)
    for use, code in zip(USES, want):
        for entry, call, accepted_too in entries(lib, desc.d, use):
            if (code == WS and not accepted_too) or skip(entry):
                continue
            got[(use, entry)] = (call(), code)
    return got


@pytest.mark.parametrize("name, v, want", ROWS, ids=[r[0] for r in ROWS])
def test_every_entry_gives_the_row_its_code(name, v, want):
    lib = L.load()
    table = status_table(lib, name, v, want)
    assert len(table) >= 12, name
    wrong = {k: r for k, r in table.items() if r[0] != r[1]}
    assert not wrong, (name, wrong, lib.teo_last_error())
    # teo_llama_decode_begin embeds a token and reads no layer weights: every variant reaches its workspace check
    d = Desc(v)
    assert lib.teo_llama_decode_begin(C.byref(d.d), C.byref(_loop_state(L.DecodeState())), FAKE, 0, None) == WS, name


def test_the_table_covers_every_entry_point_that_reads_the_layer_weights():
    """every export whose first argument is a LLaMA descriptor is called by the table, or named here with why it is not"""
    lib = L.load()
    d = Desc(variant()).d
    called = {e for use in USES for e, _, _ in entries(lib, d, use)} | {"teo_llama_decode_begin"}
    no_weights = {"teo_llama_prefill_workspace_bytes", "teo_llama_prefill_workspace_status", "teo_llama_decode_workspace_bytes",
                  "teo_llama_decode_batch_workspace_bytes", "teo_llama_decode_stream_workspace_bytes", "teo_llama_verify_workspace_bytes",
                  "teo_kv_fork"}
    sigs = {**L._SIGS, **L._SIGS_PREFIX, **L._SIGS_SCORE, **L._SIGS_GUIDE, **L._SIGS_SHARE}
    takes_desc = {n for n, (_, args) in sigs.items() if args and args[0] == C.POINTER(L.LlamaDesc)}
    assert takes_desc == called | no_weights and not called & no_weights
    assert {code for _, _, want in ROWS for code in want} == {ARG, UNS, WS}
    for i, use in enumerate(USES):                       # every use sees an accepted row, a TEO_ERR_ARG row and (where it has one) an UNS row
        assert {ARG, WS} <= {want[i] for _, _, want in ROWS}, use
