"""A vocabulary that is not a multiple of 4 through every tail (decode_tail_body plain and STREAM, verify_select_kernel; csrc/misc.hip).

The reference's builder adds 2, 4 or 6 special tokens and resizes the embeddings (videollava/model/builder.py:142-147): 32002, 32004 or
32006 rows.  The tails index row b of the fp32 logits at logits + b * vocab, read it as float4 and finish with a scalar remainder loop,
so at such a width rows b >= 1 leave 16-byte alignment, the remainder loop runs, and the sampler takes its register form on row 0 and its
radix form on the rows behind it -- inside one step.  Every other model-level test uses 300, 512 or 32000.

The configuration is tinyC515 of tests/test_containment_gpu.py: tinyC's shapes and anchor construction at vocab_size 515 = 4 x 128 + 3
with the 16 anchors on ids 499 .. 514, so the successor cycle walks THROUGH the remainder columns 512, 513 and 514 (on the CPU oracle, fp32
and bf16 alike: the prompts below, which end on anchors 8, 10 and 4, continue 9 10 11 12 13 14 15 0 1 / 11 12 13 14 15 0 15 0 1 /
5 6 7 8 9 15 0 1 2 with top-2 margins of 1.6 .. 4.0 at the three last columns).  bf16 takes the tiled skinny step, fp32 the row loop.

Nothing here has a tolerance.  Greedy: the token a step writes for row b is the FIRST index of the maximum of a host copy of d_logits[b].
Sampled: it is what teo_sample_topk draws from a fresh, 16-byte aligned copy of that row with the same seed and draw index (the equality of
the sampler's two forms is the library's contract, tests/test_kernels_gpu.py::test_sampler_register_form_draws_what_the_radix_form_draws)."""
import pytest
import torch

from teochat_amd import _lib as L
from tests import _gpu as G
from tests.test_containment_gpu import RAGGED_VOCAB, _LOCAL_TINY, _engine, _first_max

pytestmark = pytest.mark.gpu

V = RAGGED_VOCAB
BASE = _LOCAL_TINY["tinyC515"][1]["base"]
ENTRIES = (8, 10, 4)                                       # the anchors the three prompts end on
STEPS = 8
SAMPLERS = {"greedy": None, "topk20-topp0.9": dict(top_k=20, top_p=0.9), "whole-vocabulary": dict(top_k=0, top_p=1.0)}
TEMPERATURE = 1.0
SEEDS = (1234, 77, 4321)


def _prompts():
    out = []
    for i, entry in enumerate(ENTRIES):
        g = torch.Generator().manual_seed(100 + i)
        ids = torch.randint(3, BASE, (6 + 5 * i,), generator=g)
        ids[0] = 1
        ids[-1] = BASE + entry
        out.append(ids)
    return out


def _embeds(eng):
    return [eng.embed[ids.to(eng.device)] for ids in _prompts()]


def _draw(row, sampler, seed, draw):
    """teo_sample_topk on a fresh aligned copy of one logits row"""
    row = row.clone()
    assert row.is_contiguous() and row.data_ptr() % 16 == 0 and row.numel() == V
    tok = torch.zeros(1, dtype=torch.int64, device=row.device)
    L.check(G.lib().teo_sample_topk(G.p(row), G.p(tok), V, TEMPERATURE, sampler["top_k"], sampler["top_p"], int(seed), int(draw), G.stream()),
            "teo_sample_topk")
    return int(tok.item())


class _Seen:
    """where the host-side maxima of the compared rows landed (the condition on the reference, taken from the logits)"""

    def __init__(self):
        self.row0 = self.behind = self.rows = self.misaligned = 0

    def check_row(self, what, logits, b, token, sampler, rng):
        row = logits[b]
        assert bool(torch.isfinite(row).all()), what
        self.rows += 1
        self.misaligned += row.data_ptr() % 16 != 0
        want = _first_max(row.cpu())
        if want >= 512:
            self.row0 += b == 0
            self.behind += b >= 1
        if sampler is not None:
            want = _draw(row, sampler, rng[0], rng[1])
        assert int(token) == want, what + ("row", b, "token", int(token), "expected", want)


def _kw(sampler):
    return {} if sampler is None else dict(do_sample=True, temperature=TEMPERATURE, top_k=sampler["top_k"], top_p=sampler["top_p"])


@pytest.mark.parametrize("sampler", list(SAMPLERS), ids=list(SAMPLERS))
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_decode_step_at_a_ragged_vocabulary(variant, sampler):
    """teo_llama_decode_step: one row, aligned -- the float4 loop and the remainder loop of the plain tail"""
    eng, smp, seen = _engine(variant, "tinyC515"), SAMPLERS[sampler], _Seen()
    eng.reset_cache()
    first = _first_max(eng.prefill(_embeds(eng)[0], last_only=True)[0].cpu())
    eng.decode_begin(first, seed=SEEDS[0], draws_done=1, **_kw(smp))
    for step in range(STEPS):
        rng = eng.d_rng.tolist()
        eng.decode_steps(1, use_graph=False)
        seen.check_row(("teo_llama_decode_step", variant, sampler, step), eng.d_logits.view(1, V), 0, eng.d_token.item(), smp, rng)
        assert eng.generated()[-1].item() == eng.d_token.item()
    if smp is None:
        assert seen.row0 >= 1, "the maximum never landed on a remainder column"
    else:
        assert eng.d_rng.tolist() == [SEEDS[0], 1 + STEPS]
    eng.reset_cache()


def _batch_like(what, variant, sampler, stream):
    from teochat_amd.batch import BatchDecoder
    from teochat_amd.stream import StreamDecoder
    eng, smp, seen = _engine(variant, "tinyC515"), SAMPLERS[sampler], _Seen()
    embs, B = _embeds(eng), len(ENTRIES)
    if stream:
        dec = StreamDecoder(eng, B, max_new=64)
        bd = dec.bd
        lg = dec.refill(list(range(B)), embs)
        dec.configure(**_kw(smp))
        for b in range(B):
            dec.arm(b, _first_max(lg[b].cpu()), seed=SEEDS[b], limit=2 * STEPS)
    else:
        dec = bd = BatchDecoder(eng, B, max_new=64)
        lg = bd.prefill_all(embs)
        bd.begin([_first_max(lg[b].cpu()) for b in range(B)], seeds=SEEDS, draws_done=1, **_kw(smp))
    assert bd.tiled == (variant == "bf16")
    for step in range(STEPS):
        rng = bd.d_rng.tolist()
        dec.steps(1, use_graph=False)
        torch.cuda.synchronize()
        for b in range(B):
            seen.check_row((what, variant, sampler, step), bd.d_logits, b, bd.d_token[b].item(), smp, rng[b])
            assert bd.d_out[b, step].item() == bd.d_token[b].item()
    assert bd.d_pos.tolist() == [int(e.shape[0]) + STEPS for e in embs] and seen.misaligned == 2 * STEPS
    if smp is None:
        assert seen.row0 >= 1 and seen.behind >= 1, ("the maximum never landed on a remainder column", seen.row0, seen.behind)
    else:
        assert bd.d_rng.tolist() == [[SEEDS[b], 1 + STEPS] for b in range(B)]


@pytest.mark.parametrize("sampler", list(SAMPLERS), ids=list(SAMPLERS))
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_decode_batch_step_at_a_ragged_vocabulary(variant, sampler):
    """teo_llama_decode_batch_step, B = 3: rows 1 and 2 of the logits are 4-byte aligned only"""
    _batch_like("teo_llama_decode_batch_step", variant, sampler, stream=False)


@pytest.mark.parametrize("sampler", list(SAMPLERS), ids=list(SAMPLERS))
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_decode_stream_step_at_a_ragged_vocabulary(variant, sampler):
    """teo_llama_decode_stream_step, B = 3: the STREAM form of the same tail"""
    _batch_like("teo_llama_decode_stream_step", variant, sampler, stream=True)


@pytest.mark.parametrize("sampler", list(SAMPLERS), ids=list(SAMPLERS))
@pytest.mark.parametrize("variant", ["bf16", "fp32"])
def test_verify_step_at_a_ragged_vocabulary(variant, sampler):
    """teo_llama_verify_step, R = 4: the history holds the anchor cycle, so the proposer drafts the +1 walk and the tokens behind rows
    1 .. 3 are emitted whenever the model follows it.  Emitted token i of a step is the selection behind row i."""
    from teochat_amd.speculative import SpecDecoder
    eng, smp, seen = _engine(variant, "tinyC515"), SAMPLERS[sampler], _Seen()
    R = 4
    spec = SpecDecoder(eng, R, max_new=64)
    ids = _prompts()[0]
    first = _first_max(spec.prefill(eng.embed[ids.to(eng.device)])[0].cpu())
    cycle = list(range(BASE, V))
    history = cycle + cycle[:cycle.index(first) + 1] if first in cycle else ids.tolist() + [first]
    spec.begin(first, history, seed=SEEDS[0], draws_done=1, max_new=64, **_kw(smp))
    done = 0
    for step in range(STEPS):
        rng = spec.d_rng.tolist()
        now = spec.steps(1, use_graph=False)
        torch.cuda.synchronize()
        emitted = spec.generated()[done:now].tolist()
        assert 1 <= len(emitted) <= R
        for i, tok in enumerate(emitted):
            seen.check_row(("teo_llama_verify_step", variant, sampler, step), spec.d_logits, i, tok, smp, (rng[0], rng[1] + i))
        done = now
    assert not spec.stopped()
    if smp is None:
        assert seen.row0 >= 1 and seen.behind >= 1 and seen.misaligned >= 1, ("the maximum never landed on a remainder column", seen.row0, seen.behind)
        assert spec.stats()["accepted"] >= 1
    else:
        assert spec.d_rng.tolist() == [SEEDS[0], 1 + done]
