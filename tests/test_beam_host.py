"""Beam search in the device decode loop, host side (no GPU): the eighth header (include/teo_hip_beam.h) and its binding, the keyword
refusals of generate(), and the numpy restatement of the search (tests/_beam_ref.py, what tests/test_beam_gpu.py holds the kernels to)
against `transformers`' GenerationMixin.generate(num_beams=B), sequences and sequences_scores bit for bit."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from tests import _beam_ref as BR
from tests.test_containment_table import arena, declared_functions, problems, reason

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teo_hip_beam.h")
GPU = "tests/test_beam_gpu.py"
TABLE = {
    "teo_beam_state_sizeof": reason("host only: returns a number, takes no device pointer"),
    "teo_beam_select": arena(GPU),
    "teo_kv_reorder_tail": arena(GPU),
    "teo_llama_decode_beam_step": arena(GPU),
    "teo_llama_decode_beam_graph_create": reason("the same launches as the beam step beside it, which tests/test_beam_gpu.py runs: only the capture differs"),
}
SEVEN = ("teo_hip.h", "teo_hip_prefix.h", "teo_hip_score.h", "teo_hip_guide.h", "teo_hip_share.h", "teo_hip_logprob.h", "teo_hip_rules.h")
FIELDS = ["num_beams", "max_new", "eos", "early_stopping", "length_penalty", "d_len_norm", "d_scores", "d_parent", "d_token", "d_pos",
          "d_hist_token", "d_hist_parent", "d_fin_score", "d_fin_step", "d_fin_parent", "d_fin_token", "d_fin_count", "d_step", "d_done",
          "d_cand_score", "d_cand_token", "d_best_score", "d_best_flat"]


def test_the_eighth_header_is_declared_bound_and_exported():
    header = open(HEADER).read()
    assert problems(header, table=TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_BEAM) == sorted(L.EXPORTS_BEAM) == sorted(TABLE)
    others = set(L._SIGS) | set(L._SIGS_PREFIX) | set(L._SIGS_SCORE) | set(L._SIGS_GUIDE) | set(L._SIGS_SHARE) | set(L._SIGS_LOGPROB) \
        | set(L._SIGS_RULES)
    assert not set(names) & others, "a name of the eighth header is in another table"
    for h in SEVEN:
        assert f'#include "{h}"' in header, h                  # it includes the other seven ...
        assert "teo_hip_beam.h" not in open(os.path.join(ROOT, "include", h)).read(), h           # ... and none of them includes it
    for name in ("common.h", "ops.h", "runtime.h", "guide_dev.h", "share_dev.h", "logprob_dev.h", "rules_dev.h", "logprob_body.h"):
        assert "teo_hip_beam.h" not in open(os.path.join(ROOT, "teochat_amd", "csrc", name)).read(), name
    main = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    assert "#define TEO_ABI_VERSION 4" in main and L.ABI_VERSION == 4
    assert [f[0] for f in L.BeamState._fields_] == FIELDS
    mk = open(os.path.join(ROOT, "teochat_amd", "csrc", "Makefile")).read()
    assert " beam.hip" in mk and "teo_hip_beam.h" in mk and "fast-math" not in mk and "-ffast" not in mk
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for name in names:
            assert hasattr(lib, name), name
        assert lib.teo_beam_state_sizeof() == C.sizeof(L.BeamState) == 168
        # host-visible argument errors come back before any launch (no device is needed to see them)
        one = (C.c_longlong * 4)()
        a = C.addressof(one)
        good = dict(num_beams=2, max_new=4, eos=3, early_stopping=0, length_penalty=1.0, **{f: a for f in FIELDS if f.startswith("d_")})
        for bad in [dict(num_beams=1), dict(num_beams=17), dict(max_new=0), dict(early_stopping=3), dict(early_stopping=-1), dict(eos=-2),
                    dict(eos=8)] + [{f: None} for f in FIELDS if f.startswith("d_") and f != "d_pos"]:
            s = L.BeamState(**dict(good, **bad))
            assert lib.teo_beam_select(a, 8, 2, 8, C.byref(s), None) == -1, bad
        s = L.BeamState(**good)
        assert lib.teo_beam_select(None, 8, 2, 8, C.byref(s), None) == -1            # null logits
        assert lib.teo_beam_select(a, 7, 2, 8, C.byref(s), None) == -1               # ld below vocab
        assert lib.teo_beam_select(a, 8, 3, 8, C.byref(s), None) == -1               # n_rows neither 1 nor num_beams
        assert lib.teo_beam_select(a, 3, 2, 3, C.byref(s), None) == -1               # vocab below 2 * num_beams
        assert lib.teo_beam_select(a, 8, 2, 8, None, None) == -1                     # null state
        assert lib.teo_kv_reorder_tail(None, a, 2, 0, 1, None, 64, None) == -1
        d = L.LlamaDesc()
        assert lib.teo_kv_reorder_tail(C.byref(d), None, 2, 0, 1, None, 64, None) == -1
        assert lib.teo_llama_decode_beam_step(None, None, None, None, 1, None, 0, None) == -1
        assert lib.teo_llama_decode_beam_graph_create(None, None, None, None, 1, None, 0, None, None) == -1


# ---- tests/_beam_ref.py against transformers -------------------------------------------------------------------------------------------
def _table_model(table):
    T = pytest.importorskip("transformers")
    from transformers.modeling_outputs import CausalLMOutput

    class Cfg(T.PretrainedConfig):
        model_type = "beam_table"

        def __init__(self, vocab_size=8, **kw):
            super().__init__(**kw)
            self.vocab_size = vocab_size

    class TableLM(T.PreTrainedModel, T.GenerationMixin):
        """logits of the next token = a row of a seeded fp32 table indexed by the last token"""
        config_class = Cfg
        main_input_name = "input_ids"

        def __init__(self, config, tab):
            super().__init__(config)
            self.table = torch.nn.Parameter(tab.clone(), requires_grad=False)

        def forward(self, input_ids=None, attention_mask=None, **kw):
            return CausalLMOutput(logits=self.table[input_ids])

        def prepare_inputs_for_generation(self, input_ids, **kw):
            return {"input_ids": input_ids}

    return TableLM(Cfg(vocab_size=int(table.shape[0])), table)


def _make_table(V, seed, variant, eos, last):
    """variant 0: plain (runs to the length limit without an EOS); 1: EOS likely everywhere (finishes early); 2: EOS among the best of the
    first step only"""
    g = torch.Generator().manual_seed(seed)
    tab = torch.randn(V, V, generator=g) * 2.5
    if eos is not None:
        if variant == 1:
            tab[:, eos] += 7.0
        elif variant == 2:
            tab[last, eos] = tab[last].max() + 0.5
    return tab


def _ref_run(tab, prompt, B, eos, max_new, lp, es, nret, pad):
    """tests/_beam_ref.py on the table, with the tie conditions: (sequences, scores, steps, facts), or None when a tie was met"""
    facts = dict(tie=False, eos_first=False)

    def logprob_fn(seqs):
        last = torch.tensor([(s[-1] if s else prompt[-1]) for s in seqs])
        return torch.log_softmax(tab[last], dim=-1).numpy()

    def on_step(st):
        top = st["top_keys"]
        top = top[top > -np.inf]
        if np.any(top[1:] == top[:-1]):
            facts["tie"] = True
        fs = [f[0] for f in st["fin"]]
        if any(a == b for a, b in zip(fs, fs[1:])):
            facts["tie"] = True
        if st["step"] == 1 and st["fin"]:
            facts["eos_first"] = True

    seqs, scores, steps = BR.beam_search(logprob_fn, B=B, eos=eos, max_new=max_new, length_penalty=lp, early_stopping=es,
                                         num_return_sequences=nret, pad=pad, on_step=on_step)
    return seqs, scores, steps, facts


GRID = list(itertools.product((1, 2, 9), (0.0, 1.0, 2.0, -1.0), (False, True, "never"), (False, True), (False, True)))


@pytest.mark.parametrize("V", [40, 300])
@pytest.mark.parametrize("B", [2, 4, 5])
def test_the_numpy_search_is_transformers_beam_search(B, V):
    pytest.importorskip("transformers")
    prompt = [1, 2, 3]
    seen = dict(early=0, limit=0, eos_first=0, cases=0)
    for i, (max_new, lp, es, all_ret, with_eos) in enumerate(GRID):
        eos = 7 if with_eos else None
        nret = B if all_ret else 1
        variant = i % 3
        # the tie rule is ours: the seed is the first whose reference run meets no tie (chosen here, on the CPU; no case is skipped)
        for seed in range(1000 * B + V + i, 1000 * B + V + i + 50):
            tab = _make_table(V, seed, variant, eos, prompt[-1])
            ref = _ref_run(tab, prompt, B, eos, max_new, lp, es, nret, 0)
            if not ref[3]["tie"]:
                break
        seqs, scores, steps, facts = ref
        assert not facts["tie"], (i, "no seed without a tie")
        model = _table_model(tab)
        out = model.generate(torch.tensor([prompt]), num_beams=B, do_sample=False, max_new_tokens=max_new, num_return_sequences=nret,
                             use_cache=False, eos_token_id=eos, pad_token_id=0, return_dict_in_generate=True, output_scores=True,
                             length_penalty=lp, early_stopping=es)
        want = out.sequences[:, len(prompt):].numpy()
        assert want.shape == seqs.shape and np.array_equal(want, seqs), (i, max_new, lp, es, nret, eos, want, seqs)
        got_s, want_s = scores.view(np.int32), out.sequences_scores.numpy().view(np.int32)
        assert np.array_equal(got_s, want_s), (i, max_new, lp, es, nret, eos, scores, out.sequences_scores)
        seen["cases"] += 1
        seen["early"] += steps < max_new
        seen["limit"] += steps == max_new and max_new > 1
        seen["eos_first"] += facts["eos_first"] and eos is not None and max_new > 1
    assert seen["cases"] == len(GRID) == 144 and seen["early"] >= 5 and seen["limit"] >= 5 and seen["eos_first"] >= 5, seen


def test_the_numpy_step_on_hand_cases():
    ln = BR.len_norm_table(3, 1.0)
    assert ln.tolist() == [1.0, 1.0, 2.0, 3.0] and BR.len_norm_table(2, -1.0).tolist() == [1.0, 1.0, 0.5]
    lp = np.log(np.array([[0.1, 0.4, 0.2, 0.3]], np.float32))
    c, (tok, par, sc), st = BR.beam_step(lp, BR.new_state(2), B=2, eos=1, max_new=3, len_norm=ln)
    assert [x[2] for x in c] == [1, 3, 2, 0] and tok.tolist() == [3, 2] and par.tolist() == [0, 0] and not st["done"]
    assert [(f[1], f[2], f[3]) for f in st["fin"]] == [(0, 0, 1)] and st["fin"][0][0] == lp[0, 1]
    # equal keys: the lower flat index first, within a row and across rows; NaN and -inf are no candidates
    lp2 = np.array([[-1.0, -1.0, np.nan, -np.inf], [-1.0, -9.0, -9.0, -9.0]], np.float32)
    st["scores"] = np.zeros(2, np.float32)
    c, (tok, par, sc), st2 = BR.beam_step(lp2, st, B=2, eos=-1, max_new=3, len_norm=ln)
    assert [(x[1], x[2]) for x in c] == [(0, 0), (0, 1), (1, 0), (1, 1)] and tok.tolist() == [0, 1] and par.tolist() == [0, 0]
    # the last step: every candidate stops, the first B finish, the search ends
    c, _, st3 = BR.beam_step(lp2, dict(st2, scores=np.zeros(2, np.float32)), B=2, eos=-1, max_new=3, len_norm=ln)
    assert st3["done"] and len(st3["fin"]) == 2 and st3["step"] == 3
    assert BR.backtrack([[5, 6], [7, 8]], [[0, 0], [1, 0]], 2, 0, 9) == [6, 7, 9]


# ---- the keywords ----------------------------------------------------------------------------------------------------------------------
class _StubEngine:
    """records whether generate() reached the existing single-conversation path"""
    class cfg:
        vocab_size = 64
    max_seq = 32

    class _Phase:
        def __enter__(self):
            return None

        def __exit__(self, *a):
            return False

    def phase(self):
        return self._Phase()

    def guide_end(self):
        pass

    logprobs_end = rules_end = guide_end


def test_keyword_refusals_and_the_path_with_one_beam():
    from teochat_amd.beam import check_beam_args
    from teochat_amd.model import LlavaLlamaForCausalLM
    assert check_beam_args(None) is None and check_beam_args(1) is None and check_beam_args(1, num_return_sequences=1) is None
    assert check_beam_args(4) == (4, 1, 1.0, 0) and check_beam_args(4, 4, 2.0, "never") == (4, 4, 2.0, 2)
    assert check_beam_args(2, None, None, True) == (2, 1, 1.0, 1)
    for b in (0, -1, 17):
        with pytest.raises(ValueError, match="num_beams"):
            check_beam_args(b)
    with pytest.raises(ValueError, match="num_return_sequences"):
        check_beam_args(4, 5)
    with pytest.raises(ValueError, match="num_return_sequences"):
        check_beam_args(1, 2)
    with pytest.raises(ValueError, match="early_stopping"):
        check_beam_args(4, early_stopping="sometimes")
    with pytest.raises(ValueError, match="do_sample"):
        check_beam_args(4, do_sample=True)
    m = LlavaLlamaForCausalLM.__new__(LlavaLlamaForCausalLM)
    m.engine = _StubEngine()
    m.generation_config = type("G", (), {})()
    m.config = type("Cfg", (), dict(eos_token_id=2, pad_token_id=None))()
    ids = torch.ones(1, 4, dtype=torch.long)
    crit = type("Crit", (), dict(keyword_id_lists=[[5, 6]], __call__=lambda self, a, b: False))()
    for kw, match in ((dict(num_beams=0), "num_beams"), (dict(num_beams=17), "num_beams"), (dict(num_beams=4, num_return_sequences=5), "num_return"),
                      (dict(num_beams=4, do_sample=True), "do_sample"), (dict(num_beams=4, prompt_lookup_num_tokens=4), "prompt_lookup"),
                      (dict(num_beams=4, guide=object()), "guide"), (dict(num_beams=4, logprobs=True), "logprobs"),
                      (dict(num_beams=4, prefix_key="k"), "prefix_key"), (dict(num_beams=4, repetition_penalty=1.2), "logit rules"),
                      (dict(num_beams=4, no_repeat_ngram_size=2), "logit rules"), (dict(num_beams=4, min_new_tokens=2), "logit rules"),
                      (dict(num_beams=4, suppress_tokens=[3]), "logit rules"), (dict(num_beams=4, stopping_criteria=[crit]), "stop"),
                      (dict(num_beams=4, max_new_tokens=40), "max_seq")):
        with pytest.raises(ValueError, match=match):
            m.generate(input_ids=ids, **kw)
    with pytest.raises(ValueError, match="one conversation"):
        m.generate(input_ids=torch.ones(2, 4, dtype=torch.long), num_beams=4)
    # num_beams unset or 1: the existing path, which asks the (stub) model for its multimodal inputs first
    for kw in (dict(), dict(num_beams=1), dict(num_beams=1, num_return_sequences=1)):
        with pytest.raises(AttributeError, match="get_model|image_tower|prepare|model"):
            m.generate(input_ids=ids, max_new_tokens=2, **kw)
    p = inspect.signature(m._generate).parameters
    assert all(p[k].default is None for k in ("num_beams", "num_return_sequences", "length_penalty", "early_stopping"))


def test_inference_and_eval_switches():
    from teochat_amd import eval as E
    from teochat_amd import inference as I
    assert inspect.signature(I.run_inference_single).parameters["num_beams"].default is None
    a = vars(E.cli_parser().parse_args(["--dataset_name", "x", "--model_path", "y"]))
    assert "num_beams" not in a
    b = vars(E.cli_parser().parse_args(["--dataset_name", "x", "--model_path", "y", "--num_beams", "4"]))
    assert b["num_beams"] == 4
    assert inspect.signature(E.eval).parameters["num_beams"].default is None
