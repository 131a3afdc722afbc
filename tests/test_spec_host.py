"""Prompt-lookup speculative decoding, host side (no GPU): the proposer's definition (teochat_amd/speculative.py::propose_ngram), the
acceptance rule as a pure function on hand cases, and the new surface of the built library."""
import ctypes
import os
import random

import pytest

from teochat_amd import _lib as L
from teochat_amd.speculative import accept_run, propose_ngram

IMG = -200                                                  # an image sentinel as the caller passes it


def test_no_match_gives_no_drafts():
    assert propose_ngram([1, 2, 3, 4, 5], rows=4) == []
    assert propose_ngram([], rows=4) == [] and propose_ngram([7], rows=4) == []
    assert propose_ngram([1, 2, 1, 2], rows=1) == []        # one row: the pending token alone


def test_a_bigram_match_beats_a_later_unigram_match():
    #    0  1  2  3  4  5  6  7   tail = (5, 6): bigram at 0..1 -> 7 8 9; the unigram 6 also occurs later, at 5 -> 3
    h = [5, 6, 7, 8, 9, 6, 3, 4, 5, 6]
    assert propose_ngram(h, rows=4, ngram_max=2) == [7, 8, 9]
    assert propose_ngram(h, rows=4, ngram_max=1) == [3, 4, 5]
    assert propose_ngram(h, rows=2, ngram_max=2) == [7]


def test_the_most_recent_occurrence_wins():
    h = [1, 2, 10, 11, 1, 2, 20, 21, 1, 2]
    assert propose_ngram(h, rows=3) == [20, 21]
    assert propose_ngram(h, rows=8) == [20, 21, 1, 2]       # ... and runs to the end of the history


def test_a_continuation_stops_at_a_sentinel_and_at_the_end():
    assert propose_ngram([3, 4, 9, IMG, 8, 3, 4], rows=6) == [9]
    assert propose_ngram([3, 4, IMG, 8, 3, 4], rows=6) == []            # a match whose first follower is a sentinel: no draft
    assert propose_ngram([3, 4, 9, 3, 4], rows=6) == [9, 3, 4]           # end of the history
    assert propose_ngram([IMG, 5, 6, 7, IMG, 5], rows=4, ngram_max=2) == [6, 7]     # (IMG, 5) itself matches as a bigram


def test_a_continuation_may_overlap_the_tail():
    assert propose_ngram([7, 7, 7], rows=5) == [7]                        # bigram (7, 7) at 0 -> follower index 2
    assert propose_ngram([1, 2, 1, 2, 1], rows=6) == [2, 1]               # (2, 1) at 1..2 -> 2 1
    assert propose_ngram([4, 4], rows=3, ngram_max=2) == [4]              # no earlier bigram; unigram 4 at 0 -> 4


def test_propose_ngram_against_a_brute_force_model():
    rng = random.Random(11)
    for _ in range(300):
        h = [rng.choice([1, 2, 3, IMG]) for _ in range(rng.randint(0, 40))]
        rows, nmax = rng.randint(1, 8), rng.randint(1, 3)
        want = []
        for n in range(nmax, 0, -1):
            starts = [s for s in range(len(h) - n) if h[s:s + n] == h[len(h) - n:]] if len(h) > n else []
            if starts:
                f = h[starts[-1] + n:starts[-1] + n + rows - 1]
                want = f[:next((i for i, t in enumerate(f) if t < 0), len(f))]
                break
        assert propose_ngram(h, rows, nmax) == want, (h, rows, nmax)


# ---- the acceptance rule: selected[i] is what the model selects behind row i; row 0 is the pending token, row i the draft i - 1
def test_acceptance_counts_the_leading_agreement_and_adds_the_models_own_token():
    assert accept_run([5, 6, 7, 8], [5, 6, 7]) == ([5, 6, 7, 8], 3, False)            # all drafts right: R tokens
    assert accept_run([5, 6, 9, 8], [5, 6, 7]) == ([5, 6, 9], 2, False)               # right for two, then the model's own 9
    assert accept_run([4, 6, 7, 8], [5, 6, 7]) == ([4], 0, False)                     # first draft wrong: a plain step
    assert accept_run([4, 6, 7, 8], []) == ([4], 0, False)                            # no drafts: a plain step
    assert accept_run([5, 1, 7, 8], [5, 6, 7]) == ([5, 1], 1, False)                  # a later agreement (7) does not count


def test_a_stop_sequence_inside_an_accepted_run_cuts_it():
    # stop = (6, 7): completed by the third emitted token although four were accepted
    assert accept_run([5, 6, 7, 8, 9], [5, 6, 7, 8], stop_ids=[6, 7]) == ([5, 6, 7], 3, True)
    # the stop suffix may begin in an earlier step
    assert accept_run([7, 8], [7], stop_ids=[6, 7], emitted_before=[1, 6]) == ([7], 1, True)
    assert accept_run([7, 8], [9], stop_ids=[6, 7], emitted_before=[1, 6]) == ([7], 0, True)
    assert accept_run([5, 6], [5], stop_ids=[2], emitted_before=[]) == ([5, 6], 1, False)


def test_max_new_reached_mid_run_cuts_it():
    assert accept_run([5, 6, 7, 8], [5, 6, 7], emitted_before=[1, 2], max_new=4) == ([5, 6], 2, True)
    assert accept_run([5, 6, 7, 8], [5, 6, 7], emitted_before=[1, 2], max_new=6) == ([5, 6, 7, 8], 3, True)
    assert accept_run([5, 6, 7, 8], [5, 6, 7], emitted_before=[1, 2], max_new=7) == ([5, 6, 7, 8], 3, False)
    assert accept_run([5], [], emitted_before=[1, 2], max_new=2) == ([], 0, True)      # nothing left to emit


def test_the_stream_does_not_depend_on_the_drafts():
    """Run a deterministic 'model' (next token = f(all tokens so far)) with perfect, wrong and random drafts: the same stream, and the
    step counts of the issue -- ceil((n - 1) / R) with perfect drafts, n - 1 with wrong ones."""
    def model(ctx):
        return (sum(ctx[-3:]) * 7 + len(ctx)) % 11

    def run(drafter, R, n):
        ctx, out, steps, pending = [3, 1, 4], [], 0, None
        pending = model(ctx)                                   # the prefill's token
        out.append(pending)
        while len(out) < n:
            drafts = drafter(ctx, pending, out)[:R - 1]
            rows = [pending] + drafts
            sel = [model(ctx + rows[:i + 1]) for i in range(len(rows))]
            em, _, _ = accept_run(sel, drafts, emitted_before=out, max_new=n)
            ctx += rows[:len(em)]
            out += em
            pending = em[-1]
            steps += 1
        return out, steps

    n = 23
    plain, steps_plain = run(lambda c, p, o: [], 4, n)
    assert steps_plain == n - 1
    perfect, steps = run(lambda c, p, o: plain[len(o):], 4, n)
    assert perfect == plain and steps == -(-(n - 1) // 4)
    wrong, steps = run(lambda c, p, o: [(t + 1) % 11 for t in plain[len(o):]], 4, n)
    assert wrong == plain and steps == n - 1
    rng = random.Random(5)
    noisy, _ = run(lambda c, p, o: [t if rng.random() < 0.6 else 0 for t in plain[len(o):]], 6, n)
    assert noisy == plain


# ---- the library
def test_the_verify_attention_is_exported_declared_and_bound():
    assert os.path.exists(L.LIB_PATH), "libteo_hip.so missing: run __graft_entry__.build()"
    lib = ctypes.CDLL(L.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "teo_hip.h")).read()
    for name in ("teo_attn_verify", "teo_attn_verify_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS and name + "(" in hdr, name
    for name in ("teo_llama_verify_workspace_bytes", "teo_llama_verify_begin", "teo_llama_verify_step", "teo_llama_verify_step_profile",
                 "teo_llama_verify_graph_create", "teo_spec_propose"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTS and name + "(" in hdr, name
    lib.teo_sizeof.restype, lib.teo_sizeof.argtypes = ctypes.c_size_t, [ctypes.c_char_p]
    assert lib.teo_sizeof(b"teo_verify_state") == ctypes.sizeof(L.VerifyState) > 0
    b = L.load().teo_attn_verify_workspace_bytes
    assert b(32, 128, 4096, 8) == L.load().teo_attn_decode_workspace_bytes(32, 128, 4096, 8) > 0
    assert b(32, 128, 4096, 0) == 0
