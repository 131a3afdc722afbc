"""Token log-probabilities, host side (no GPU): the sixth header (include/teo_hip_logprob.h) and its binding, the keyword rules of
generate() / generate_stream(), teochat_amd/confidence.py on the byte tokenizer, and the switches of inference / eval with a stub model."""
import ctypes as C
import inspect
import math
import os

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import confidence as CF
from teochat_amd import inference as I
from tests.test_containment_table import arena, declared_functions, problems, reason
from tests.test_stream_host import StubProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teo_hip_logprob.h")
CONTAINMENT = "tests/test_logprob_gpu.py"
STEP = reason("an existing step's launches followed by teo_logprob_record, which tests/test_logprob_gpu.py runs on arenas")
TABLE = {
    "teo_logprob_rec_sizeof": reason("host only: returns a number, takes no device pointer"),
    "teo_logprob_rows": arena(CONTAINMENT),
    "teo_logprob_record": arena(CONTAINMENT),
    "teo_llama_decode_step_logp": STEP, "teo_llama_decode_graph_create_logp": STEP,
    "teo_llama_decode_batch_step_logp": STEP, "teo_llama_decode_batch_graph_create_logp": STEP,
    "teo_llama_decode_stream_step_logp": STEP, "teo_llama_decode_stream_graph_create_logp": STEP,
}


def test_the_sixth_header_has_a_table_and_a_binding_of_its_own():
    header = open(HEADER).read()
    assert problems(header, table=TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_LOGPROB) == sorted(L.EXPORTS_LOGPROB) == sorted(TABLE)
    others = set(L._SIGS) | set(L._SIGS_PREFIX) | set(L._SIGS_SCORE) | set(L._SIGS_GUIDE) | set(L._SIGS_SHARE)
    assert not set(names) & others, "a name of the sixth header is in another table"
    assert '#include "teo_hip.h"' in header
    for name in ("include/teo_hip.h", "include/teo_hip_prefix.h", "include/teo_hip_score.h", "include/teo_hip_guide.h", "include/teo_hip_share.h",
                 "teochat_amd/csrc/common.h", "teochat_amd/csrc/ops.h", "teochat_amd/csrc/guide_dev.h", "teochat_amd/csrc/share_dev.h",
                 "teochat_amd/csrc/runtime.h"):
        assert "teo_hip_logprob.h" not in open(os.path.join(ROOT, name)).read(), name            # nothing existing includes it
    main = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    assert "#define TEO_ABI_VERSION 4" in main and L.ABI_VERSION == 4
    assert [f[0] for f in L.LogprobRec._fields_] == ["d_logprobs", "stride", "d_rec_count", "top_k", "d_top_ids", "d_top_logprobs"]
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for name in names:
            assert hasattr(lib, name), name
        assert lib.teo_logprob_rec_sizeof() == C.sizeof(L.LogprobRec) == 48
        # host-visible argument errors come back before any launch (no device is needed to see them)
        assert lib.teo_logprob_rows(None, 0, 0, 0, None, None, None, None, 0, None) == -1
        assert lib.teo_logprob_record(None, 0, 0, 0, None, 0, None, None, None) == -1
        one = (C.c_int * 4)()
        for bad in (dict(top_k=9), dict(top_k=2, d_top_ids=None), dict(stride=0), dict(d_logprobs=None), dict(d_rec_count=None)):
            r = L.LogprobRec(C.addressof(one), 1, C.addressof(one), 0, C.addressof(one), C.addressof(one))
            for k, v in bad.items():
                setattr(r, k, v)
            assert lib.teo_logprob_record(None, 0, 0, 0, None, 0, None, C.byref(r), None) == -1, bad
        assert lib.teo_llama_decode_step_logp(None, None, None, None, None, 0, None) == -1
        assert lib.teo_llama_decode_batch_step_logp(None, None, None, None, 0, None) == -1
        assert lib.teo_llama_decode_stream_step_logp(None, None, None, None, None, None, 0, None) == -1


def test_keyword_rules():
    from teochat_amd.model import LlavaLlamaForCausalLM, check_logprob_args
    assert check_logprob_args(True, 0) == 0 and check_logprob_args(True, 8) == 8 and check_logprob_args(False, 0) == 0
    assert check_logprob_args(None, None) == 0
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        check_logprob_args(True, 0, 4)
    for k in (-1, 9):
        with pytest.raises(ValueError, match="outside 0..8"):
            check_logprob_args(True, k)
    with pytest.raises(ValueError, match="needs logprobs=True"):
        check_logprob_args(False, 3)
    # generate / generate_batch / generate_stream refuse before they touch the engine
    m = LlavaLlamaForCausalLM.__new__(LlavaLlamaForCausalLM)
    ids = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        m.generate(input_ids=ids, logprobs=True, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match="outside 0..8"):
        m.generate(input_ids=ids, logprobs=True, top_logprobs=9)
    with pytest.raises(ValueError, match="needs logprobs=True"):
        m.generate(input_ids=ids, top_logprobs=2)
    with pytest.raises(ValueError, match="needs logprobs=True"):
        m.generate_stream([ids[0]], top_logprobs=2)
    with pytest.raises(ValueError, match="outside 0..8"):
        m.generate_batch([ids[0]], logprobs=True, top_logprobs=-1)
    for fn in (m._generate, m._generate_batch, m._generate_stream):
        p = inspect.signature(fn).parameters
        assert p["logprobs"].default is False and p["top_logprobs"].default == 0


def byte_ids(text):
    return [3 + b for b in text.encode()]


def test_confidence_on_the_byte_tokenizer():
    from teochat_amd.guide import pieces_of
    from teochat_amd.tokenizer_stub import ByteTokenizer
    pieces = pieces_of(ByteTokenizer(), vocab=300)
    assert CF.answer_confidence([0.0] * 5) == 1.0 and CF.answer_confidence(torch.zeros(1, 4)) == 1.0
    assert abs(CF.answer_confidence([math.log(0.5), math.log(0.125), float("nan")]) - 0.25) < 1e-12
    text = "two: [1, 22, 3, 4] and then [50, 6, 7, 88]."
    ids = byte_ids(text) + [2]                                             # the stop token: no piece, inside no box
    lp = [-0.01 * (i + 1) for i in range(len(ids))]
    got = CF.box_confidences(pieces, ids, lp)
    assert [b for b, _ in got] == I.extract_bboxes(text) == [[1, 22, 3, 4], [50, 6, 7, 88]]
    for (box, conf), sub in zip(got, ("[1, 22, 3, 4]", "[50, 6, 7, 88]")):
        lo = text.index(sub)
        inside = lp[lo:lo + len(sub)]                                      # exactly the tokens from the opening [ to the closing ]
        assert abs(conf - math.exp(sum(inside) / len(inside))) < 1e-12
    assert CF.box_confidences(pieces, byte_ids("no box here") + [2], [-1.0] * 12) == []
    cut = "[1, 2, 3, 4], [5, 6, 7"                                         # the second box is cut off by max_new_tokens
    assert [b for b, _ in CF.box_confidences(pieces, byte_ids(cut), [-0.5] * len(cut))] == [[1, 2, 3, 4]]
    rec = CF.confidence_record(pieces, torch.tensor(ids), torch.tensor(lp))
    assert sorted(rec) == ["box_confidences", "confidence", "logprobs"] and len(rec["logprobs"]) == len(ids)
    assert rec["box_confidences"][0][0] == [1, 22, 3, 4] and 0 < rec["confidence"] < 1


class LogprobStub:
    """generate / generate_batch / generate_stream as the model has them with logprobs=True: request i is answered with a box and
    log-probabilities of -0.1 per token"""
    device, dtype = "cpu", torch.float32

    def __init__(self, tokenizer):
        from types import SimpleNamespace
        self.tok, self.calls, self.config = tokenizer, [], SimpleNamespace(vocab_size=300)

    def _answer(self, i, ids):
        ans = torch.tensor(self.tok(f"[1, 2, 3, {i}]</s>").input_ids[1:], dtype=ids.dtype)
        return torch.cat([ids.view(-1), ans]), torch.full((ans.numel(),), -0.1)

    def generate(self, input_ids=None, images=None, logprobs=False, **kw):
        from teochat_amd.model import GenerateOutput
        self.calls.append(("generate", logprobs))
        seq, lp = self._answer(len(self.calls) - 1, input_ids[0])
        return GenerateOutput(seq.view(1, -1), lp.view(1, -1)) if logprobs else seq.view(1, -1)

    def _many(self, name, ids_list, logprobs):
        self.calls.append((name, logprobs))
        outs = [self._answer(i, ids_list[i]) for i in range(len(ids_list))]
        return [(s, lp, None, None) for s, lp in outs] if logprobs else [s for s, _ in outs]

    def generate_batch(self, input_ids_list, images_list=None, logprobs=False, **kw):
        return self._many("batch", input_ids_list, logprobs)

    def generate_stream(self, input_ids_list, images_list=None, logprobs=False, **kw):
        return self._many("stream", input_ids_list, logprobs)


def _examples(n=4):
    return [{"conversations": [{"value": f"<video>\nquestion {i}"}, {"value": f"gt [5, 6, 7, {i}]"}], "video": [f"img{i}"], "timestamp": [],
             "task": "det", "polygon": [[i, 0]]} for i in range(n)]


@pytest.mark.parametrize("mode", ["single", "groups", "continuous"])
def test_records_carry_confidence_and_box_confidences(mode):
    from teochat_amd.tokenizer_stub import ByteTokenizer
    tok = ByteTokenizer()
    kw = {"single": {}, "groups": dict(batch_size=2), "continuous": dict(batch_size=2, continuous=True)}[mode]
    model = LogprobStub(tok)
    plain = I.run_inference(_examples(), model, tok, StubProcessor(), "interleave", True, "v1", 0.2, 64, **kw)
    assert all("confidence" not in r and "box_confidences" not in r for r in plain) and not any(c[1] for c in model.calls)
    model = LogprobStub(tok)
    outs = I.run_inference(_examples(), model, tok, StubProcessor(), "interleave", True, "v1", 0.2, 64, logprobs=True, **kw)
    assert all(c[1] for c in model.calls)
    for r, p in zip(outs, plain):
        assert {k: v for k, v in r.items() if k not in ("confidence", "box_confidences")}.keys() == p.keys()
        assert abs(r["confidence"] - math.exp(-0.1)) < 1e-6
        assert len(r["box_confidences"]) == 1 and r["box_confidences"][0][0][:3] == [1, 2, 3]
        assert abs(r["box_confidences"][0][1] - math.exp(-0.1)) < 1e-6
    if mode == "single":
        text, info = I.run_inference_single(model, StubProcessor(), tok, "<video>\nq", ["a"], return_logprobs=True)
        assert text.startswith("[1, 2, 3,") and sorted(info) == ["box_confidences", "confidence", "logprobs"]
        assert inspect.signature(I.run_inference_single).parameters["return_logprobs"].default is False
        assert list(inspect.signature(I.run_inference_single).parameters)[-1] == "return_logprobs"
    # the metrics functions ignore the new keys
    from teochat_amd.detection import detection_metrics
    import copy
    stripped = [{k: v for k, v in r.items() if k not in ("confidence", "box_confidences")} for r in copy.deepcopy(outs)]
    try:
        want = detection_metrics(stripped, dataset_name="xbd_loc")
    except Exception:                                                      # (the metric needs more than these records hold: nothing to compare)
        return
    assert detection_metrics(outs, dataset_name="xbd_loc") == want


def test_eval_cli_logprobs_flag_is_off_and_absent_by_default():
    from teochat_amd import eval as E
    base = ["--dataset_name", "x", "--model_path", "y"]
    assert "logprobs" not in vars(E.cli_parser().parse_args(base))
    assert vars(E.cli_parser().parse_args(base + ["--logprobs"]))["logprobs"] is True
    assert inspect.signature(E.eval).parameters["logprobs"].default is False
    assert inspect.signature(I.run_inference).parameters["logprobs"].default is False
    assert inspect.signature(I.run_inference_batch).parameters["logprobs"].default is False
