"""Logit rules in the device decode loop, host side (no GPU): the seventh header (include/teo_hip_rules.h) and its binding, the keyword
refusals of generate() / generate_batch() / generate_stream(), and the numpy restatement of the four rules (tests/_rules_ref.py, what
tests/test_rules_gpu.py holds the kernel to) against the `transformers` logits processors, bit for bit."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from tests import _rules_ref as RR
from tests.test_containment_table import arena, declared_functions, problems, reason

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "teo_hip_rules.h")
GPU = "tests/test_rules_gpu.py"
CAPTURE = reason("the same launches as the ruled step beside it, which tests/test_rules_gpu.py runs on arenas: only the capture differs")
TABLE = {
    "teo_logit_rules_sizeof": reason("host only: returns a number, takes no device pointer"),
    "teo_logit_rules_seed": arena(GPU),
    "teo_logit_rules_apply": arena(GPU),
    "teo_llama_decode_step_ruled": arena(GPU),
    "teo_llama_decode_graph_create_ruled": CAPTURE,
    "teo_llama_decode_stream_step_ruled": arena(GPU),
    "teo_llama_decode_stream_graph_create_ruled": CAPTURE,
}
SIX = ("teo_hip.h", "teo_hip_prefix.h", "teo_hip_score.h", "teo_hip_guide.h", "teo_hip_share.h", "teo_hip_logprob.h")


def test_the_seventh_header_is_declared_bound_and_exported():
    header = open(HEADER).read()
    assert problems(header, table=TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_RULES) == sorted(L.EXPORTS_RULES) == sorted(TABLE)
    others = set(L._SIGS) | set(L._SIGS_PREFIX) | set(L._SIGS_SCORE) | set(L._SIGS_GUIDE) | set(L._SIGS_SHARE) | set(L._SIGS_LOGPROB)
    assert not set(names) & others, "a name of the seventh header is in another table"
    for h in SIX:
        assert f'#include "{h}"' in header, h                  # it includes the other six ...
        assert "teo_hip_rules.h" not in open(os.path.join(ROOT, "include", h)).read(), h          # ... and none of them includes it
    for name in ("common.h", "ops.h", "runtime.h", "guide_dev.h", "share_dev.h", "logprob_dev.h"):
        assert "teo_hip_rules.h" not in open(os.path.join(ROOT, "teochat_amd", "csrc", name)).read(), name
    main = open(os.path.join(ROOT, "include", "teo_hip.h")).read()
    assert "#define TEO_ABI_VERSION 4" in main and L.ABI_VERSION == 4
    assert [f[0] for f in L.LogitRules._fields_] == ["repetition_penalty", "no_repeat_ngram", "min_new", "vocab", "d_flags", "d_hist",
                                                     "d_hist_len", "hist_stride"]
    assert (L.RULE_SEEN, L.RULE_BANNED, L.RULE_EOS) == (RR.SEEN, RR.BANNED, RR.EOS_BIT) == (1, 2, 4)
    mk = open(os.path.join(ROOT, "teochat_amd", "csrc", "Makefile")).read()
    assert " rules.hip" in mk and "teo_hip_rules.h" in mk and "fast-math" not in mk and "-ffast" not in mk
    if os.path.exists(L.LIB_PATH):
        lib = L.load()
        for name in names:
            assert hasattr(lib, name), name
        assert lib.teo_logit_rules_sizeof() == C.sizeof(L.LogitRules) == 48
        # host-visible argument errors come back before any launch (no device is needed to see them)
        one = (C.c_longlong * 4)()
        a = C.addressof(one)
        good = dict(repetition_penalty=1.2, no_repeat_ngram=2, min_new=1, vocab=4, d_flags=a, d_hist=a, d_hist_len=a, hist_stride=2)
        for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram=-1),
                    dict(min_new=-1), dict(vocab=0), dict(hist_stride=0), dict(d_flags=None), dict(d_hist=None), dict(d_hist_len=None)):
            r = L.LogitRules(**dict(good, **bad))
            assert lib.teo_logit_rules_apply(a, 4, 1, C.byref(r), None, None, None, None) == -1, bad
            assert lib.teo_logit_rules_seed(C.byref(r), 0, None, 0, None) == -1, bad
        r = L.LogitRules(**good)
        assert lib.teo_logit_rules_apply(None, 4, 1, C.byref(r), None, None, None, None) == -1           # null logits
        assert lib.teo_logit_rules_apply(a, 3, 1, C.byref(r), None, None, None, None) == -1              # ld below vocab
        assert lib.teo_logit_rules_apply(a, 4, 1, None, None, None, None, None) == -1                    # null rules
        assert lib.teo_logit_rules_seed(C.byref(r), 0, a, 3, None) == -1                                 # more ids than the history holds
        assert lib.teo_logit_rules_seed(C.byref(r), 0, None, 1, None) == -1 and lib.teo_logit_rules_seed(C.byref(r), -1, a, 1, None) == -1
        assert lib.teo_llama_decode_step_ruled(None, None, None, None, None, None, 0, None) == -1
        assert lib.teo_llama_decode_stream_step_ruled(None, None, None, None, None, None, None, 0, None) == -1


def test_keyword_refusals():
    from teochat_amd.decode_host import check_rule_args, rule_args_ban
    from teochat_amd.model import LlavaLlamaForCausalLM
    for neutral in (dict(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[])):
        assert check_rule_args(**neutral) is None
    assert check_rule_args(1.2, 3, 8, [5, 3, 5], vocab=10) == (1.2, 3, 8, [3, 5])
    assert not rule_args_ban(check_rule_args(1.3)) and rule_args_ban(check_rule_args(None, 2)) and rule_args_ban(check_rule_args(None, None, 1))
    assert rule_args_ban(check_rule_args(suppress_tokens=[1])) and not rule_args_ban(None)
    for p in (0, 0.0, -1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            check_rule_args(p)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        check_rule_args(None, -1)
    with pytest.raises(ValueError, match="min_new_tokens"):
        check_rule_args(None, None, -2)
    for sup in ([10], [3, -1]):
        with pytest.raises(ValueError, match="outside the vocabulary"):
            check_rule_args(suppress_tokens=sup, vocab=10)
    # generate / generate_batch / generate_stream refuse before they touch the engine
    m = LlavaLlamaForCausalLM.__new__(LlavaLlamaForCausalLM)
    ids = torch.ones(1, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="repetition_penalty"):
        m.generate(input_ids=ids, repetition_penalty=0)
    with pytest.raises(ValueError, match="repetition_penalty"):
        m.generate_stream([ids[0]], repetition_penalty=-1)
    with pytest.raises(ValueError, match="no_repeat_ngram_size"):
        m.generate(input_ids=ids, no_repeat_ngram_size=-1)
    with pytest.raises(ValueError, match="min_new_tokens"):
        m.generate_stream([ids[0]], min_new_tokens=-1)
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(min_new_tokens=8), dict(suppress_tokens=[7])):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            m.generate(input_ids=ids, prompt_lookup_num_tokens=4, **kw)
        with pytest.raises(ValueError, match="generate_stream"):
            m.generate(input_ids=torch.ones(2, 4, dtype=torch.long), **kw)
        with pytest.raises(ValueError, match="generate_stream"):
            m.generate_batch([ids[0], ids[0]], **kw)
    guide = object()                              # (refused before the guide is looked at)
    for kw in (dict(no_repeat_ngram_size=2), dict(min_new_tokens=1), dict(suppress_tokens=[7])):
        with pytest.raises(ValueError, match="not combined with a guide"):
            m.generate(input_ids=ids, guide=guide, **kw)
        with pytest.raises(ValueError, match="not combined with a guide"):
            m.generate_stream([ids[0]], guides=[guide], **kw)
    for fn in (m._generate, m._generate_stream):
        p = inspect.signature(fn).parameters
        assert all(p[k].default is None for k in ("repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "suppress_tokens"))


def _hf(seq, x, p=1.0, n=0, selected=0, m=0, eos=(), suppress=(), prompt_len=0):
    """HF's order of the processors in GenerationMixin._get_logits_processor: repetition penalty, no-repeat n-gram, min new tokens,
    suppress"""
    LP = pytest.importorskip("transformers").generation.logits_process
    ids = torch.tensor([seq], dtype=torch.long)
    s = torch.from_numpy(x.copy()).view(1, -1)
    if p != 1.0:
        s = LP.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
    if n > 0:
        s = LP.NoRepeatNGramLogitsProcessor(n)(ids, s)
    if m > 0 and eos:
        s = LP.MinNewTokensLengthLogitsProcessor(prompt_len, m, list(eos), device="cpu")(ids, s)
    if suppress:
        s = LP.SuppressTokensLogitsProcessor(list(suppress), device="cpu")(ids, s)
    return s[0].numpy()


@pytest.mark.parametrize("V", [259, 301])
def test_the_numpy_rules_are_the_transformers_processors(V):
    pytest.importorskip("transformers")
    rng = np.random.default_rng(V)
    cases = 0
    for trial in range(6):
        x = RR.edge_row(V, rng)
        prompt_len = int(rng.integers(1, 6))
        new = int(rng.integers(0, 7))
        # a small alphabet, so that n-grams repeat; ids of the edge values (+-0, -inf, huge) are in the sequence too
        alphabet = list(rng.permutation(V)[:5]) + [int(i) for i in np.flatnonzero(~np.isfinite(x) | (x == 0) | (np.abs(x) > 1e30))[:4]]
        seq = [int(alphabet[i]) for i in rng.integers(0, len(alphabet), prompt_len + new)]
        eos, sup = [int(alphabet[0]), V - 1], [0, int(alphabet[1]), V - 2]
        for p in (0.7, 1.0, 1.3):
            for n in (0, 1, 2, 4):
                for m in (0, new, new + 1):
                    got = RR.np_rules(x, seq, p=p, n=n, selected=new, m=m, eos=eos, suppress=sup)
                    want = _hf(seq, x, p=p, n=n, selected=new, m=m, eos=eos, suppress=sup, prompt_len=prompt_len)
                    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (trial, p, n, m)
                    cases += 1
        # every rule alone
        for kw in (dict(p=1.3), dict(p=0.7), dict(n=1), dict(n=2), dict(n=3), dict(m=new + 1, eos=eos), dict(suppress=sup)):
            got = RR.np_rules(x, seq, selected=new, **kw)
            want = _hf(seq, x, selected=new, prompt_len=prompt_len, **kw)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (trial, kw)
    assert cases == 6 * 36


def test_the_numpy_rules_on_hand_cases():
    x = np.array([1.0, -2.0, 0.0, -0.0, -np.inf, 4.0, 8.0, np.nan], np.float32)
    out = RR.np_rules(x, [0, 1, 2, 3, 4, 7, -200], p=2.0)
    assert np.array_equal(out[:7].view(np.int32), np.array([0.5, -4.0, 0.0, -0.0, -np.inf, 4.0, 8.0], np.float32).view(np.int32))
    assert out.view(np.int32)[7] == x.view(np.int32)[7]                                  # a NaN keeps its bits; the sentinel addresses nothing
    # n = 2: the sequence ends on 5; every earlier 5 bans its follower.  A sentinel compares like any id and is never banned itself
    assert np.flatnonzero(np.isneginf(RR.np_rules(np.zeros(8, np.float32), [5, 1, 5, 6, -200, 5, -200, 5], n=2))).tolist() == [1, 6]
    assert np.flatnonzero(np.isneginf(RR.np_rules(np.zeros(8, np.float32), [1, 2], n=4))).tolist() == []          # L + 1 < n
    assert np.flatnonzero(np.isneginf(RR.np_rules(np.zeros(8, np.float32), [1, 2, 3], n=4))).tolist() == []       # L + 1 == n: no follower yet
    assert np.flatnonzero(np.isneginf(RR.np_rules(np.zeros(8, np.float32), [1, 2, 3, 7, 1, 2, 3], n=4))).tolist() == [7]
    assert np.flatnonzero(np.isneginf(RR.np_rules(np.zeros(8, np.float32), [3, 3, -200, 6], n=1))).tolist() == [3, 6]
    assert np.isneginf(RR.np_rules(np.zeros(8, np.float32), [], selected=2, m=3, eos=[2]))[2]
    assert not np.isneginf(RR.np_rules(np.zeros(8, np.float32), [], selected=3, m=3, eos=[2])).any()
    assert RR.np_flags(8, [1, -200, 3], eos=[2], suppress=[3]).tolist() == [0, 1, 4, 3, 0, 0, 0, 0]


def test_inference_and_eval_switches():
    """run_inference_single / run_inference hand the two keywords on only when they are given, and the eval flags are absent by default"""
    from teochat_amd import eval as E
    from teochat_amd import inference as I
    for fn in (I.run_inference_single, I.run_inference):
        p = inspect.signature(fn).parameters
        assert p["repetition_penalty"].default is None and p["no_repeat_ngram_size"].default is None, fn.__name__
    a = vars(E.cli_parser().parse_args(["--dataset_name", "x", "--model_path", "y"]))
    assert "repetition_penalty" not in a and "no_repeat_ngram_size" not in a
    b = vars(E.cli_parser().parse_args(["--dataset_name", "x", "--model_path", "y", "--repetition_penalty", "1.2", "--no_repeat_ngram_size", "3"]))
    assert b["repetition_penalty"] == 1.2 and b["no_repeat_ngram_size"] == 3
    params = inspect.signature(E.eval).parameters
    assert params["repetition_penalty"].default is None and params["no_repeat_ngram_size"].default is None
