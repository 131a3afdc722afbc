"""Prompt-lookup speculative decoding through generate(prompt_lookup_num_tokens=K) and SpecDecoder on the GPU: the tokens are the
non-speculative stream whatever the drafts are (golden streams of the reference in fp32, seeded sampling, stops), the step counts
follow the acceptance rule, and in bf16 -- where the verify step streams the weights through the batched step's GEMMs, not the GEMVs --
the greedy tokens agree with the plain loop's at every decisive position of the anchored synthetic checkpoint."""
import math

import pytest
import torch

from oracle import teo_oracle as O
from teochat_amd.speculative import SpecDecoder, propose_ngram
from tests import _tiny as TY
from tests.test_model_gpu import FP32_TOL, build, inputs

pytestmark = pytest.mark.gpu

NAMES = ["tinyA", "tinyB", "tinyC"]


def _conv(name):
    g = TY.load_npz(name)
    model, _ = build(name, torch.float32)
    frames, ids = inputs(name, g)
    dev = model.device
    return g, model, ids.to(dev), [f.to(dev) for f in frames]


def _embeds(model, ids, imgs):
    (_, _, _, _, emb, _) = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, imgs)
    return emb[0]


@pytest.mark.parametrize("name", NAMES)
def test_generate_with_prompt_lookup_returns_the_golden_stream(name):
    g, model, ids, imgs = _conv(name)
    want = g["greedy_tokens"].tolist()
    n = len(want)
    for K in (1, 3, 7):
        out = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=n, eos_token_id=None, prompt_lookup_num_tokens=K)
        assert out[0, :ids.shape[1]].tolist() == ids[0].tolist()
        assert out[0, ids.shape[1]:].tolist() == want, (name, K)
        st = model.last_generation_stats
        # every step emits its accepted drafts and one token of the model's own, except a last one that max_new cuts inside its run
        assert st["emitted"] == n - 1 and 1 <= st["steps"] <= n - 1 and 0 <= st["accepted"] - (n - 1 - st["steps"]) <= 1, (name, K, st)
        assert model._spec_decoder.R == K + 1
    if name == "tinyC":
        assert len(set(want)) == 8                            # the stream that leaves the +1 walk: eight distinct tokens
    # the logits behind the last token: a step-by-step run (host drafts = the proposer's definition) against the reference's last step
    R = 4
    spec = SpecDecoder(model.engine, R, max_new=64, draft_source=lambda h: propose_ngram(h, R, 2))
    first = int(spec.prefill(_embeds(model, ids, imgs))[0].argmax())
    assert first == want[0]
    spec.begin(first, ids[0].tolist() + [first], max_new=n - 1)
    done = 0
    while not spec.stopped():
        now = spec.steps(1)
        last_row = now - done - 1                             # the row whose selection is the last emitted token
        done = now
    assert [first] + spec.generated().tolist() == want
    d = float((spec.d_logits[last_row].cpu() - torch.from_numpy(g["greedy_logits"][-1])).abs().max())
    print(f"[{name}] verify-step logits behind the last token: max abs diff vs reference {d:.2e}")
    assert d < FP32_TOL


@pytest.mark.parametrize("name", ["tinyB", "tinyC"])
def test_step_counts_follow_the_drafts(name):
    """Drafts injected from a prior plain run: perfect -> ceil((n - 1) / (K + 1)) steps; all wrong -> n - 1 steps, none accepted; right
    for j tokens and then wrong -> exactly j accepted per step.  The tokens are the plain stream every time."""
    g, model, ids, imgs = _conv(name)
    n = 13
    plain = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=n, eos_token_id=None)[0, ids.shape[1]:].tolist()
    V = model.engine.cfg.vocab_size
    emb = _embeds(model, ids, imgs)
    P = ids.shape[1]

    def run(K, drafter):
        spec = SpecDecoder(model.engine, K + 1, max_new=64, draft_source=lambda h: drafter(len(h) - P))
        first = int(spec.prefill(emb)[0].argmax())
        spec.begin(first, ids[0].tolist() + [first], max_new=n - 1)
        while not spec.stopped():
            spec.steps(4)
        return [first] + spec.generated().tolist(), spec.stats()

    for K in (1, 3, 7):
        toks, st = run(K, lambda m: plain[m:m + K])                               # m tokens so far; the pending one is plain[m - 1]
        assert toks == plain and st["steps"] == math.ceil((n - 1) / (K + 1)), (K, st)
        assert 0 <= st["accepted"] - (n - 1 - st["steps"]) <= 1           # (+1: a last run cut by max_new inside the accepted drafts)
        toks, st = run(K, lambda m: [(t + 1) % V for t in plain[m:m + K]])
        assert toks == plain and st["steps"] == n - 1 and st["accepted"] == 0 and st["proposed"] > 0, (K, st)
    for j in (1, 2, 3):                                                           # (n - 1) = 12 is a multiple of j + 1
        toks, st = run(7, lambda m: plain[m:m + j] + [(plain[m + j] + 1) % V] if m + j < n else plain[m:m + j])
        assert toks == plain and st["steps"] == (n - 1) // (j + 1) and st["accepted"] == j * st["steps"], (j, st)


@pytest.mark.parametrize("name", NAMES)
def test_seeded_sampling_does_not_depend_on_speculation(name):
    g, model, ids, imgs = _conv(name)
    kw = dict(input_ids=ids, images=imgs, do_sample=True, temperature=0.8, top_k=20, top_p=0.9, max_new_tokens=24, eos_token_id=None)
    plain = model.generate(generator=torch.Generator().manual_seed(7), **kw)
    for K in (2, 5):
        spec = model.generate(generator=torch.Generator().manual_seed(7), prompt_lookup_num_tokens=K, **kw)
        assert torch.equal(spec, plain), (name, K)
    other = model.generate(generator=torch.Generator().manual_seed(8), prompt_lookup_num_tokens=2, **kw)
    assert other.shape == plain.shape


def test_stops_cut_an_accepted_run_at_the_exact_token():
    g, model, ids, imgs = _conv("tinyC")
    n = 12
    plain = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=n, eos_token_id=None)[0, ids.shape[1]:].tolist()
    P = ids.shape[1]
    emb = _embeds(model, ids, imgs)
    # a two-id stop sequence completed by the 3rd token of an accepted run of 8 (perfect drafts)
    stop = plain[2:4]
    assert all(plain[i:i + 2] != stop for i in range(2)), "the stop sequence first completes at token 3"
    spec = SpecDecoder(model.engine, 8, max_new=64, draft_source=lambda h: plain[len(h) - P:len(h) - P + 7])
    first = int(spec.prefill(emb)[0].argmax())
    spec.begin(first, ids[0].tolist() + [first], stop_ids=stop, max_new=n - 1)
    spec.steps(3)
    assert spec.stopped() and [first] + spec.generated().tolist() == plain[:4] and spec.stats()["steps"] == 1
    assert spec.cache_len == emb.shape[0] + 3
    # through generate(): EOS inside a run, and max_new_tokens met exactly
    eos = plain[5]
    want = plain[:plain.index(eos) + 1]
    for K in (3, 7):
        out = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=n, eos_token_id=eos, prompt_lookup_num_tokens=K)
        assert out[0, P:].tolist() == want, K
        ref = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=n, eos_token_id=eos)
        assert torch.equal(out, ref)
        for m in (1, 2, 5):
            out = model.generate(input_ids=ids, images=imgs, do_sample=False, max_new_tokens=m, eos_token_id=None, prompt_lookup_num_tokens=K)
            assert out[0, P:].tolist() == plain[:m], (K, m)


def test_argument_errors_and_the_option_off():
    g, model, ids, imgs = _conv("tinyB")
    want = g["greedy_tokens"].tolist()
    kw = dict(input_ids=ids, images=imgs, do_sample=False, eos_token_id=None)
    out = model.generate(max_new_tokens=len(want), prompt_lookup_num_tokens=0, **kw)
    assert out[0, ids.shape[1]:].tolist() == want
    out = model.generate(max_new_tokens=len(want), prompt_lookup_num_tokens=None, **kw)
    assert getattr(model, "_spec_decoder", None) is None, "K = 0 / None is today's path: no SpecDecoder"
    for K in (16, -1, 40):
        with pytest.raises(ValueError):
            model.generate(max_new_tokens=4, prompt_lookup_num_tokens=K, **kw)
    L_ = _embeds(model, ids, imgs).shape[0]
    room = model.engine.max_seq - L_                           # the plain loop takes max_new_tokens = room; K drafts need K more rows:
    with pytest.raises(ValueError):                            # prompt + max_new_tokens - 1 + (K + 1) <= max_seq
        model.generate(max_new_tokens=room - 6, prompt_lookup_num_tokens=7, **kw)
    out = model.generate(max_new_tokens=room - 7, prompt_lookup_num_tokens=7, **kw)
    assert out.shape[1] == ids.shape[1] + room - 7
    assert out[0, ids.shape[1]:ids.shape[1] + len(want)].tolist() == want
    with pytest.raises(ValueError):
        model.generate(input_ids=torch.cat([ids, ids]), images=[imgs, imgs], max_new_tokens=4, prompt_lookup_num_tokens=2)
    assert getattr(model, "_spec_decoder", None) is not None


def test_bf16_greedy_tokens_agree_at_every_decisive_position():
    """bf16 on the anchored synthetic checkpoint of tests/test_configs_gpu.py: the verify step streams the weights through the skinny
    GEMMs, not the GEMVs, so its guarantee is 'the batched kernels' greedy stream' -- compared with the plain loop at the positions
    whose top-2 margin exceeds the noise bound of those tests (their rule, on one teacher-forcing prefill over the plain stream) up to
    the first position that is not decisive, as the batched-vs-single check there does.  At least half of the positions must be
    decisive, checked on the plain loop first."""
    from tests.test_configs_gpu import _load, conversation, decisive_rows
    m = _load(1024)
    frames, ids = conversation(2, 64, seed=3)
    n = 48
    plain = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n, eos_token_id=None)[0, ids.shape[1]:].tolist()
    full = torch.cat([ids, torch.tensor([plain[:-1]], dtype=ids.dtype, device=ids.device)], dim=1)
    rows = m(input_ids=full, images=frames).logits[0][-n:]
    decisive, top1, _ = decisive_rows(rows)
    n_dec = int(decisive.sum())
    print(f"plain loop: {n_dec}/{n} positions decisive")
    assert n_dec >= n // 2, f"only {n_dec}/{n} positions decisive"
    assert bool((top1 == torch.tensor(plain, device=top1.device))[decisive].all())
    dec = decisive.tolist()
    from tests.test_configs_gpu import teacher_forced_check
    for K in (3, 7):
        spec = m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=n, eos_token_id=None,
                          prompt_lookup_num_tokens=K)[0, ids.shape[1]:].tolist()
        diff = [i for i in range(n) if spec[i] != plain[i]]
        first_diff = diff[0] if diff else n
        st = m.last_generation_stats
        print(f"K={K}: first difference from the plain stream at {first_diff} of {n}"
              + (f" (decisive there: {dec[first_diff]})" if diff else "") + f"; {st}")
        # up to the first difference both streams share one context, so the plain stream's `decisive` vector holds there: the streams
        # may only part at a position that is not decisive
        assert first_diff == n or not dec[first_diff], f"K={K}: the streams part at decisive position {first_diff}"
        # behind a legitimate near-tie split the contexts differ: the speculative stream is teacher-forced on its own (one prefill over
        # prompt + its tokens; every decisive position of ITS context must be the prefill's argmax, at least half must be decisive)
        teacher_forced_check(m, ids, frames, spec, tag=f"bf16 prompt lookup K={K}", min_decisive=0.5)
    assert m.last_generation_stats is not None
    m.generate(input_ids=ids, images=frames, do_sample=False, max_new_tokens=2, eos_token_id=None)
    assert m.last_generation_stats is None                     # a plain call leaves no stale statistics
