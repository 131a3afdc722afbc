"""Scoring answer options as packed branches, host side (no GPU): the planner of teochat_amd/score.py, the branch visibility mask fed to
the attention probes' expectation builders (with planted faults: the GPU probes of tests/test_score_gpu.py can fail), the table of the
third header (include/teo_hip_score.h) checked by the containment table's own checker, and run_inference_options with stubs."""
import os

import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import inference as I
from teochat_amd.score import PROMPT_ROW, plan_branches
from tests import _attn_probes as P
from tests.test_containment_table import arena, declared_functions, problems, reason

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_HEADER = os.path.join(ROOT, "include", "teo_hip_score.h")


# ------------------------------------------------------------------------------------------------------------------------ the planner
def options_of(lens, base=10):
    """option c = [base * (c + 1), base * (c + 1) + 1, ...]: every token says which option and which place it is"""
    return [[base * (c + 1) + k for k in range(n)] for c, n in enumerate(lens)]


def check_contract(p, past):
    """what teo_llama_prefill_branches asks of its caller, and the bookkeeping of the triples"""
    bs, pos = p["branch_start"], p["positions"]
    S = len(p["rows"])
    assert len(bs) == len(pos) == S
    for i in range(S):
        assert bs[i] == 0 if i == 0 else bs[i] in (bs[i - 1], i)
        assert pos[i] == past + i - bs[i]


def test_plan_of_five_options_in_one_pass():
    lens, past = [1, 2, 4, 66, 3], 70
    opts = options_of(lens)
    passes = plan_branches(opts, past, max_seq=1024, max_rows=1024)
    assert len(passes) == 1
    p = passes[0]
    check_contract(p, past)
    assert p["options"] == [0, 1, 2, 3, 4]
    assert p["rows"] == [t for o in opts for t in o[:-1]]                       # every option feeds all but its last token
    assert len(p["rows"]) == sum(n - 1 for n in lens) == 71
    assert p["branch_start"] == [0] + [1] * 3 + [4] * 65 + [69] * 2
    assert p["positions"] == [70] + [70, 71, 72] + list(range(70, 135)) + [70, 71]
    # the first token of every option is predicted by the prompt's last row, token k + 1 by the row that feeds token k: one triple each
    seen = {}
    for row, label, c in p["triples"]:
        k = opts[c].index(label)
        assert (c, k) not in seen
        seen[(c, k)] = row
        if k == 0:
            assert row == PROMPT_ROW
        else:
            assert p["rows"][row] == opts[c][k - 1] and p["branch_start"][row] + (k - 1) == row
    assert sorted(seen) == [(c, k) for c, n in enumerate(lens) for k in range(n)]
    assert [t[2] for t in p["triples"]] == sorted(t[2] for t in p["triples"])   # option by option, token by token


def test_plan_splits_at_max_rows_and_at_max_seq_and_never_cuts_an_option():
    lens, past = [1, 2, 4, 66, 3], 70
    opts = options_of(lens)
    # feeds 0, 1, 3, 65, 2.  max_rows = 65: [0, 1, 3] | [65] | [2]
    by_rows = plan_branches(opts, past, max_seq=1024, max_rows=65)
    assert [p["options"] for p in by_rows] == [[0, 1, 2], [3], [4]]
    assert [len(p["rows"]) for p in by_rows] == [4, 65, 2]
    # max_seq = 70 + 67: [0, 1, 3] + 65 = 69 > 67 -> [0, 1, 3] | [65, 2]
    by_seq = plan_branches(opts, past, max_seq=137, max_rows=1024)
    assert [p["options"] for p in by_seq] == [[0, 1, 2], [3, 4]]
    assert [len(p["rows"]) for p in by_seq] == [4, 67]
    for passes in (by_rows, by_seq):
        for p in passes:
            check_contract(p, past)
            assert past + len(p["rows"]) <= 1024
            for c in p["options"]:                                               # whole options only
                assert sum(1 for t in p["triples"] if t[2] == c) == lens[c]
        assert sorted(t for p in passes for t in p["triples"] if t[0] == PROMPT_ROW) == [(PROMPT_ROW, opts[c][0], c) for c in range(5)]
    # every pass numbers its rows from 0 and every branch is at the positions behind the prompt
    assert by_seq[1]["branch_start"] == [0] * 65 + [65] * 2 and by_seq[1]["positions"] == list(range(70, 135)) + [70, 71]
    # one-token options feed nothing and ride along, even with a full pass
    full = plan_branches([[5, 6, 7], [8], [9]], 10, max_seq=12, max_rows=1024)
    assert len(full) == 1 and full[0]["rows"] == [5, 6] and [t[0] for t in full[0]["triples"]] == [PROMPT_ROW, 0, 1, PROMPT_ROW, PROMPT_ROW]


def test_plan_rejects_an_option_that_cannot_fit_alone():
    opts = options_of([1, 2, 4, 66, 3])
    with pytest.raises(ValueError, match="option 3 feeds 65 rows"):
        plan_branches(opts, 70, max_seq=1024, max_rows=64)
    with pytest.raises(ValueError, match="option 3 feeds 65 rows"):
        plan_branches(opts, 70, max_seq=70 + 64, max_rows=1024)
    assert len(plan_branches(opts, 70, max_seq=70 + 65, max_rows=65)) == 3       # exactly fitting is fine
    with pytest.raises(ValueError, match="no tokens"):
        plan_branches([[1], []], 70, 1024, 1024)
    with pytest.raises(ValueError, match="at least one row"):
        plan_branches([[1]], 0, 1024, 1024)


# ------------------------------------------------------------------------------------------------------ the mask and the probes' power
LENS = [1, 3, 70, 2, 33, 64, 1]            # the GPU probes' branches: q_len 174


def branch_starts(lens):
    """branch_start of branches of these lengths packed behind each other"""
    bs = []
    for n in lens:
        bs += [len(bs)] * n
    return bs


def branch_mask(past, lens):
    """The visibility rule of teo_attn_branches as rows of booleans [sum(lens)][past + sum(lens)]: query row i sees key j iff j < past or
    past + branch_start[i] <= j <= past + i."""
    bs = branch_starts(lens)
    return [[j < past or past + bs[i] <= j <= past + i for j in range(past + len(bs))] for i in range(len(bs))]


def vis_of(past, lens):
    return torch.tensor(branch_mask(past, lens), dtype=torch.bool)


def plant(vis, past, lens, kind):
    """the branch mask with one indexing error a branch kernel can make"""
    out = vis.clone()
    bs = branch_starts(lens)
    for i in range(len(bs)):
        if kind == "last_prefix_key_dropped":
            out[i, past - 1] = False
        elif kind == "previous_branch_last_key_visible":
            if bs[i] > 0:
                out[i, past + bs[i] - 1] = True
        elif kind == "own_first_key_dropped":
            if i > bs[i] or past > 0:                         # (a one-row branch without a prefix keeps its only key)
                out[i, past + bs[i]] = False
        elif kind == "key_behind_the_diagonal_visible":
            if past + i + 1 < out.shape[1]:
                out[i, past + i + 1] = True
        else:
            raise ValueError(kind)
    return out


def window_keys_of(past, lens):
    """keys past - 1 and past, then the first and the last key of three branches with their neighbours"""
    bs = branch_starts(lens)
    starts = sorted(set(bs))
    want = [past - 1, past]
    for s in (starts[1], starts[2], starts[4]):
        e = s + lens[starts.index(s)] - 1
        want += [past + s - 1, past + s, past + s + 1, past + e - 1, past + e, past + e + 1]
    keys = []
    for j in want:
        if 0 <= j < past + sum(lens) and j not in keys:
            keys.append(j)
    return keys


def test_branch_mask_is_the_causal_mask_with_a_lower_bound_per_row():
    assert torch.equal(vis_of(70, [9]), P.visible_mask(9, 79, True))            # one branch: plain causal
    vis = vis_of(5, [2, 3])
    want = torch.zeros(5, 10, dtype=torch.bool)
    want[:, :5] = True
    for i, lo in enumerate([0, 0, 2, 2, 2]):
        want[i, 5 + lo:5 + i + 1] = True
    assert torch.equal(vis, want)
    assert branch_starts(LENS) == [0] + [1] * 3 + [4] * 70 + [74] * 2 + [76] * 33 + [109] * 64 + [173]


@pytest.mark.parametrize("kind", ["last_prefix_key_dropped", "previous_branch_last_key_visible", "own_first_key_dropped",
                                  "key_behind_the_diagonal_visible"])
def test_planted_mask_faults_change_an_expectation(kind):
    """each fault moves the expectation of at least one of the probe forms the GPU test runs: the probes can fail"""
    past, d, Hk, H = 70, 64, 1, 2
    q_len, kv = sum(LENS), 70 + sum(LENS)
    vis = vis_of(past, LENS)
    bad = plant(vis, past, LENS, kind)
    assert not torch.equal(bad, vis)
    v = P.random_v((1, Hk, kv, d), torch.bfloat16, seed=3)
    changed = []
    changed.append(not torch.equal(P.selector_expected(v, H, vis, True), P.selector_expected(v, H, bad, True)))
    changed.append(not torch.equal(P.selector_expected(v, H, vis, False), P.selector_expected(v, H, bad, False)))
    wv = P.window_v(kv, d, window_keys_of(past, LENS)).view(1, 1, kv, d)
    changed.append(not torch.equal(P.membership_expected(wv, H, vis), P.membership_expected(wv, H, bad)))
    assert any(changed), kind
    # the form that is meant to catch it
    meant = {"last_prefix_key_dropped": 2, "previous_branch_last_key_visible": 2, "own_first_key_dropped": 2, "key_behind_the_diagonal_visible": 0}
    assert changed[meant[kind]], (kind, changed)
    # dense membership at past 5, short branches: every key counts somewhere, so every fault shows
    lens = [1, 3, 20, 2, 1]
    vis5, kv5 = vis_of(5, lens), 5 + sum(lens)
    dv = P.dense_v(kv5, d, 1, True).view(1, 1, kv5, d)
    assert not torch.equal(P.membership_expected(dv, H, vis5), P.membership_expected(dv, H, plant(vis5, 5, lens, kind)))
    # descending selector at past = 0 returns the branch's first V row: dropping it moves the answer
    vis0 = vis_of(0, LENS)
    first = P.selector_expected(v[:, :, :q_len], H, vis0, False)
    assert torch.equal(first[0, 0], v[0, 0, torch.tensor(branch_starts(LENS))])
    if kind == "own_first_key_dropped":
        assert not torch.equal(first, P.selector_expected(v[:, :, :q_len], H, plant(vis0, 0, LENS, kind), False))


# ------------------------------------------------------------------------------------------------------------ the third header's table
SCORE_CONTAINMENT = "tests/test_score_gpu.py"
SCORE_TABLE = {
    "teo_attn_branches": arena(SCORE_CONTAINMENT),
    "teo_llama_prefill_branches": arena(SCORE_CONTAINMENT),
    "teo_token_logprobs": arena(SCORE_CONTAINMENT),
}


def test_the_third_header_has_a_table_and_a_binding_of_its_own():
    header = open(SCORE_HEADER).read()
    assert problems(header, table=SCORE_TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_SCORE) == sorted(L.EXPORTS_SCORE) == sorted(SCORE_TABLE)
    assert not set(names) & (set(L._SIGS) | set(L._SIGS_PREFIX)), "a name of the third header is in another table"
    assert '#include "teo_hip.h"' in header
    for name in ("include/teo_hip.h", "include/teo_hip_prefix.h", "teochat_amd/csrc/common.h", "teochat_amd/csrc/ops.h"):
        assert "teo_hip_score.h" not in open(os.path.join(ROOT, name)).read(), name           # nothing existing includes it
    lib = L.load()
    for name in names:
        assert hasattr(lib, name), name
    assert lib.teo_version() == 4 == L.ABI_VERSION
    fake = header.replace("int teo_token_logprobs(", "int teo_brand_new_kernel(const void* d_x, void* d_y, int n);\nint teo_token_logprobs(")
    assert problems(fake, table=SCORE_TABLE) == ["teo_brand_new_kernel: declared in the header, no row in the table"]
    assert problems(header, table=dict(SCORE_TABLE, teo_gone=reason("host only: a number"))) == ["teo_gone: in the table, not declared in the header"]
    short = {k: v for k, v in SCORE_TABLE.items() if k != "teo_attn_branches"}
    assert problems(header, table=short) == ["teo_attn_branches: declared in the header, no row in the table"]


# ------------------------------------------------------------------------------------------------------------- run_inference_options
class ScoringStub:
    """score_options as the model has it: records the call; option c scores -(its second id) / 10 per token."""
    device, dtype = "cpu", torch.float32

    def __init__(self):
        self.calls = []

    def score_options(self, input_ids, images, options, attention_mask=None, max_rows=1024):
        self.calls.append(dict(input_ids=input_ids.clone(), n_frames=len(images), options=[list(o) for o in options]))
        return torch.tensor([-0.1 * (o[0] - 3) * len(o) for o in options], dtype=torch.float32)

    def generate(self, input_ids=None, images=None, **kw):
        self.calls.append(dict(input_ids=input_ids.clone(), n_frames=len(images), generate=True))
        return torch.cat([input_ids, torch.tensor([[2]])], dim=1)


class Processor:
    def __init__(self):
        self.seen = []

    def preprocess(self, path, return_tensors="pt"):
        self.seen.append(path)
        return {"pixel_values": [torch.zeros(3, 2, 2)]}


def test_run_inference_options_ids_normalize_argmax_and_prompt():
    from teochat_amd.tokenizer_stub import ByteTokenizer
    tok = ByteTokenizer()
    model, proc = ScoringStub(), Processor()
    inp = "<video>\nWhich class is this? Answer with one of: A, AB, B."
    paths, stamps = ["img_a", "img_b"], ["2019-05-01", "2017-01-15"]
    options = ["A", "AB", "B"]
    best, scores = I.run_inference_options(model, proc, tok, inp, paths, options, timestamps=stamps)
    call = model.calls[-1]
    # ids: the tokenizer's, without the leading BOS, plus EOS -- "A" is not a prefix of "AB" any more
    A, B = 3 + ord("A"), 3 + ord("B")
    assert call["options"] == [[A, 2], [A, B, 2], [B, 2]]
    assert I.option_token_ids(ByteTokenizer(add_bos=False), "AB") == [A, B, 2]
    # scores -0.1 * (first id - 3) * tokens: A -> -13.0, AB -> -19.5, B -> -13.2
    assert scores.dtype == torch.float32 and scores.tolist() == pytest.approx([-13.0, -19.5, -13.2], rel=1e-6)
    assert best == "A"
    best_n, scores_n = I.run_inference_options(model, proc, tok, inp, paths, options, timestamps=stamps, normalize=True)
    assert scores_n.tolist() == pytest.approx([-6.5, -6.5, -6.6], rel=1e-6)
    assert torch.equal(scores_n, scores / torch.tensor([2.0, 3.0, 2.0])) and best_n == options[int(scores_n.argmax())]
    flipped = ScoringStub()
    flipped.score_options = lambda input_ids, images, options, **kw: torch.tensor([-3.0, -1.0, -2.0])
    assert I.run_inference_options(flipped, proc, tok, inp, paths, options)[0] == "AB"
    # the prompt, the frames and their chronological order are run_inference_single's
    proc.seen.clear()
    I.run_inference_single(model, proc, tok, inp, paths, timestamps=stamps, do_sample=False, max_new_tokens=1)
    single = model.calls[-1]
    assert single.get("generate") and torch.equal(single["input_ids"], call["input_ids"]) and single["n_frames"] == call["n_frames"] == 2
    assert proc.seen == ["img_b", "img_a"]
    with pytest.raises(ValueError):
        I.run_inference_options(model, proc, tok, inp, paths, [])
