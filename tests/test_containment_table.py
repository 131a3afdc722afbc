"""The table that keeps the containment suite in step with the header (host test, no GPU).

Every `teo_*` function declared in include/teo_hip.h is listed here with one of two things: the test file that calls it on guarded arenas
(tests/_arena.py), or a one-line reason why it has no device operand of its own to be contained.  A declaration added to the header without
a row here fails this test, and so does a row whose file stopped calling the entry point: tests/test_containment_gpu.py once stopped at
teo_llama_decode_batch_step while two features added entry points that own device memory between calls."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teo_hip.h")

CONTAINMENT = "tests/test_containment_gpu.py"
SPEC_ATTN = "tests/test_spec_attn_gpu.py"
STREAM = "tests/test_stream_gpu.py"


def arena(path):
    return ("arena", path)


def reason(text):
    return ("reason", text)


HOST_ONLY = reason("host only: returns a number or a string, takes no device pointer")
SAME_LAUNCHES = "the same launches as {0}, which is called on arenas: only the timing events / the capture around them differ"

TABLE = {
    # ---- strings, sizes, plans, knobs
    "teo_version": HOST_ONLY,
    "teo_last_error": HOST_ONLY,
    "teo_last_kernel": HOST_ONLY,
    "teo_gemm_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_gemm_fp8_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_gemm_w4_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_gemm_w4a8_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_gemv_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_gemv_qkv_plan": reason("host only: the planner's choice as a string, launches nothing"),
    "teo_sizeof": HOST_ONLY,
    "teo_tune_create": reason("host only: a knob block in host memory"),
    "teo_tune_destroy": reason("host only: a knob block in host memory"),
    "teo_tune_set": reason("host only: a knob block in host memory"),
    "teo_tune_get": reason("host only: a knob block in host memory"),
    "teo_tune_reset": reason("host only: a knob block in host memory"),
    "teo_tune_bind": reason("host only: a knob block in host memory"),
    "teo_tune_keys": HOST_ONLY,
    "teo_gemm_uses_mfma": reason("host only: a predicate on shapes"),
    "teo_gemm_workspace_bytes": reason("host only: a size; teo_gemm_ws runs on exactly that many bytes in " + CONTAINMENT),
    "teo_attn_decode_workspace_bytes": reason("host only: a size"),
    "teo_attn_verify_workspace_bytes": reason("host only: a size; teo_attn_verify runs on exactly that many bytes in " + SPEC_ATTN),
    "teo_vit_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_projector_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_llama_prefill_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_llama_decode_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_llama_decode_batch_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_llama_decode_stream_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    "teo_llama_verify_workspace_bytes": reason("host only: a size; the stage runs on exactly that many bytes in " + CONTAINMENT),
    # ---- kernels
    "teo_layernorm": arena(CONTAINMENT),
    "teo_rmsnorm": arena(CONTAINMENT),
    "teo_gemm": arena(CONTAINMENT),
    "teo_gemm_workspace_init": arena(CONTAINMENT),
    "teo_gemm_workspace_status": arena(CONTAINMENT),
    "teo_gemm_ws": arena(CONTAINMENT),
    "teo_gemm_fp8": arena(CONTAINMENT),
    "teo_gemm_fp8_ws": arena(CONTAINMENT),
    "teo_quant_rows_fp8": arena(CONTAINMENT),
    "teo_patch_embed": arena(CONTAINMENT),
    "teo_im2col_patches": arena(CONTAINMENT),
    "teo_vit_embed_ln": arena(CONTAINMENT),
    "teo_attention": arena(CONTAINMENT),
    "teo_vit_value_transpose": arena(CONTAINMENT),
    "teo_rope_kv_append": arena(CONTAINMENT),
    "teo_embed_splice": arena(CONTAINMENT),
    "teo_attn_decode": arena(CONTAINMENT),                    # its parked form (d_pos < 0): PARKED_FORMS below
    "teo_attn_verify": arena(SPEC_ATTN),
    "teo_cross_entropy": arena(CONTAINMENT),
    "teo_preprocess_frames": arena(CONTAINMENT),
    "teo_preprocess_frames_pad": arena(CONTAINMENT),
    "teo_drop_cls": arena(CONTAINMENT),
    "teo_argmax": arena(CONTAINMENT),
    "teo_sample_topk": arena(CONTAINMENT),
    "teo_gemv": arena(CONTAINMENT),
    "teo_gemv_w8": arena(CONTAINMENT),
    "teo_gemv_w4": arena(CONTAINMENT),
    "teo_gemm_skinny": arena(CONTAINMENT),
    "teo_gemm_skinny_w4": arena(CONTAINMENT),
    "teo_gemm_w4": arena(CONTAINMENT),
    "teo_gemm_w4a8": arena(CONTAINMENT),
    # ---- stages
    "teo_vit_encode": arena(CONTAINMENT),
    "teo_vit_workspace_status": arena(CONTAINMENT),
    "teo_projector": arena(CONTAINMENT),
    "teo_llama_prefill": arena(CONTAINMENT),
    "teo_llama_prefill_attentions": arena(CONTAINMENT),
    "teo_llama_prefill_batch": arena(CONTAINMENT),
    "teo_llama_prefill_slots": arena(CONTAINMENT),
    "teo_llama_prefill_workspace_status": arena(CONTAINMENT),
    "teo_llama_decode_begin": arena(CONTAINMENT),
    "teo_llama_decode_step": arena(CONTAINMENT),
    "teo_llama_decode_step_profile": reason(SAME_LAUNCHES.format("teo_llama_decode_step")),
    "teo_llama_decode_graph_create": reason(SAME_LAUNCHES.format("teo_llama_decode_step")),
    "teo_graph_launch": reason("replays a captured step: the operands are the ones its *_graph_create call was given"),
    "teo_graph_destroy": reason("host only: frees the graph object"),
    "teo_llama_decode_batch_begin": arena(CONTAINMENT),
    "teo_llama_decode_batch_step": arena(CONTAINMENT),
    "teo_llama_decode_batch_step_profile": reason(SAME_LAUNCHES.format("teo_llama_decode_batch_step")),
    "teo_llama_decode_batch_graph_create": reason(SAME_LAUNCHES.format("teo_llama_decode_batch_step")),
    "teo_llama_decode_stream_step": arena(CONTAINMENT),
    "teo_llama_decode_stream_graph_create": arena(CONTAINMENT),
    "teo_llama_decode_stream_arm": arena(CONTAINMENT),
    "teo_llama_verify_begin": arena(CONTAINMENT),
    "teo_llama_verify_step": arena(CONTAINMENT),
    "teo_llama_verify_step_profile": reason(SAME_LAUNCHES.format("teo_llama_verify_step")),
    "teo_llama_verify_graph_create": arena(CONTAINMENT),
    "teo_spec_propose": arena(CONTAINMENT),
    # ---- multi-GPU context
    "teo_comm_unique_id": reason("host only: 128 bytes of host memory"),
    "teo_ctx_create": reason("context creation: host objects and the communicator, no caller-owned device memory"),
    "teo_ctx_destroy": reason("host only: frees the context"),
    "teo_ctx_info": HOST_ONLY,
    "teo_ctx_tune": reason("host only: a knob block in host memory"),
    "teo_allgather_visual": reason("one collective handed to the communication library as (pointer, count): no kernel of this library "
                                   "indexes its operands, and it needs one process per GPU"),
}

# forms of an entry point that a second file covers on arenas: (name, file, a text that file must contain)
PARKED_FORMS = (("teo_attn_decode", STREAM, "test_parked_conversation_is_inert_in_attn_decode"),)


def declared_functions(header_text):
    """every teo_* function DECLARATION of the header: comments stripped, a line that starts with a return type and reaches `teo_x(`"""
    s = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    s = re.sub(r"//[^\n]*", "", s)
    return re.findall(r"(?m)^[A-Za-z_][\w \t\*]*?[ \t\*](teo_\w+)[ \t]*\(", s)


def problems(header_text, table=None, root=ROOT):
    """the list of disagreements between the header and the table (empty = fine)"""
    table = TABLE if table is None else table
    names = declared_functions(header_text)
    out = []
    if len(set(names)) != len(names):
        out.append(f"declared twice: {sorted(n for n in set(names) if names.count(n) > 1)}")
    out += [f"{n}: declared in the header, no row in the table" for n in names if n not in table]
    out += [f"{n}: in the table, not declared in the header" for n in table if n not in names]
    texts = {}
    for n, (kind, arg) in sorted(table.items()):
        if kind == "reason":
            if not (isinstance(arg, str) and len(arg.strip()) >= 10 and "\n" not in arg):
                out.append(f"{n}: the reason must be one line that says something")
            continue
        if kind != "arena":
            out.append(f"{n}: unknown kind {kind!r}")
            continue
        path = os.path.join(root, arg)
        if not os.path.isfile(path):
            out.append(f"{n}: {arg} does not exist")
            continue
        if arg not in texts:
            texts[arg] = open(path).read()
        if not re.search(r"(?m)^\s*(from tests import _arena\b|from tests\._arena import|import tests\._arena\b)", texts[arg]):
            out.append(f"{n}: {arg} does not import tests._arena")
        if not re.search(r"\b" + re.escape(n) + r"\(", texts[arg]):
            out.append(f"{n}: {arg} does not call {n}(")
    return out


def test_the_parser_reads_the_header_as_the_loader_does():
    """every export the ctypes loader binds is a declaration the parser finds, and the other way round"""
    from teochat_amd import _lib as L
    names = declared_functions(open(HEADER).read())
    assert len(names) > 80 and sorted(names) == sorted(L._SIGS.keys())


def test_every_declared_entry_point_has_a_row_and_every_row_holds():
    assert problems(open(HEADER).read()) == []
    for name, path, text in PARKED_FORMS:
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(r"(?m)^\s*from tests import _arena\b", src) and name + "(" in src and text in src, (name, path)


def test_the_table_can_fail():
    """a declaration without a row, a row without a declaration, a file that does not call its entry, a missing file: each is reported"""
    header = open(HEADER).read()
    fake = header.replace("int teo_version(void);", "int teo_version(void);\nint teo_brand_new_kernel(const void* d_x, void* d_y, int n);")
    assert problems(fake) == ["teo_brand_new_kernel: declared in the header, no row in the table"]
    short = {k: v for k, v in TABLE.items() if k != "teo_spec_propose"}
    assert problems(header, short) == ["teo_spec_propose: declared in the header, no row in the table"]
    assert problems(header, dict(TABLE, teo_gone=HOST_ONLY)) == ["teo_gone: in the table, not declared in the header"]
    assert problems(header, dict(TABLE, teo_version=arena(CONTAINMENT))) == [f"teo_version: {CONTAINMENT} does not call teo_version("]
    assert problems(header, dict(TABLE, teo_gemm=arena("tests/test_no_such_file.py"))) == ["teo_gemm: tests/test_no_such_file.py does not exist"]
    assert problems(header, dict(TABLE, teo_gemm=arena("tests/test_host_logic.py")))[0] == "teo_gemm: tests/test_host_logic.py does not import tests._arena"
    assert problems(header, dict(TABLE, teo_version=reason(""))) == ["teo_version: the reason must be one line that says something"]
