"""The verify step (teo_llama_verify_step, teochat_amd/speculative.py::SpecDecoder) on the GPU: one step against the batched step on
staggered conversations bit for bit at LLaMA-2-7B widths, the device proposer against its Python definition, and hipGraph replay against
plain launches."""
import functools
import random

import pytest
import torch

from oracle import teo_oracle as O
from teochat_amd import _lib as L
from teochat_amd.speculative import SpecDecoder, propose_ngram
from tests import _gpu as G

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.uint8)


@functools.lru_cache(maxsize=1)
def _real_width_sd():
    vit = dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=3, hidden_act="gelu")
    llm = dict(hidden_size=4096, num_attention_heads=32, num_key_value_heads=32, intermediate_size=11008, num_hidden_layers=2,
               vocab_size=32000)
    vcfg, lcfg, mm = O.VitCfg(**vit), O.LlamaCfg(**llm), O.MMCfg()
    return vit, llm, O.make_state_dict(vcfg, lcfg, mm, seed=2, std=0.02)


@functools.lru_cache(maxsize=1)
def _real_width_model(weights):
    """LLaMA-2-7B widths, 2 layers (the model of test_batched_decode_real_width_vs_single): bf16, fp8 or batch_mxfp4 decode weights."""
    from teochat_amd.config import LlavaConfig, VisionConfig
    from teochat_amd.engine import TeoEngine
    from teochat_amd.model import LlavaLlamaForCausalLM
    vit, llm, sd = _real_width_sd()
    cfg = LlavaConfig(**llm, max_position_embeddings=1024, vision_config=VisionConfig(**vit))
    eng = TeoEngine(sd, cfg, dtype=BF, device="cuda:0", max_seq=512, weight_format="mxfp4" if weights == "batch_mxfp4" else weights)
    if weights == "batch_mxfp4":
        eng.set_options(batch_mxfp4=True)
    return LlavaLlamaForCausalLM(cfg, eng)


@pytest.mark.parametrize("R", [4, 8])
@pytest.mark.parametrize("weights", ["native", "fp8", "batch_mxfp4"])
def test_verify_step_is_bitwise_the_staggered_batched_step(weights, R):
    """One verify step over rows = [pending, drafts...] at positions P .. P + R - 1 against BatchDecoder(batch = R): d_logits row i and the
    K / V / V^T rows appended at P + i, in every layer, bit for bit.

    The reference conversations are staggered by the batched step itself: all R slots hold the prompt, step t feeds slot i the token
    rows[min(t, i)], and slot t's logits and appended row are taken at step t -- when it is fed rows[t] at position P + t with rows
    P .. P + t - 1 of its cache appended by the earlier steps.  (Rows a PREFILL appends come from other GEMM kernels -- with fp8 or MXFP4
    decode weights from other weights -- and cannot be the bits a decode step appends; the contract of teo_attn_verify is 'as the
    earlier rows would have appended them'.)  At R = 8 x 32 heads the batched step's attention is the whole-context kernel, at R = 4 the
    split pair: the verify kernel follows either through the shared chunk rule."""
    model = _real_width_model(weights)
    eng = model.engine
    V = eng.cfg.vocab_size
    ids = O.synthetic_prompt_ids(24, 0, V, seed=41)
    P = int(ids.numel())
    g = torch.Generator().manual_seed(100 + R)
    rows = torch.randint(3, V, (R,), generator=g).tolist()                  # the pending token and R - 1 injected drafts
    emb = model.get_model().embed_tokens(ids.view(1, -1).to(DEV))[0]
    dec = model.batch_decoder(R, 16)
    assert dec.tiled and dec.w4 == (weights == "batch_mxfp4")
    dec.reset()
    for b in range(R):
        dec.prefill(b, emb)
    ref_logits, ref_k, ref_v, ref_vt = [], [], [], []
    for t in range(R):
        lg = dec.forward_step([rows[min(t, i)] for i in range(R)])
        ref_logits.append(lg[t].clone())
        ref_k.append(dec.k_cache[:, t, :, P + t].clone())                   # [layers, Hk, hd]
        ref_v.append(dec.v_cache[:, t, :, P + t].clone())
        ref_vt.append(dec.vt_cache[:, t, :, :, P + t].clone())
    spec = SpecDecoder(eng, R, max_new=16, draft_source=lambda hist: rows[1:], batch_decoder=dec)
    assert (spec.state.w_tiled, spec.state.w_mxfp4) == (1, int(weights == "batch_mxfp4"))
    for c in (spec.k_cache, spec.v_cache, spec.vt_cache):
        c.fill_(float("nan"))                                                # nothing behind the context may matter
    spec.prefill(emb)
    spec.begin(rows[0], ids.tolist() + [rows[0]], max_new=8)
    assert spec.d_rows.tolist() == rows and int(spec.d_n_draft.item()) == R - 1
    spec.steps(1)
    got = spec.d_logits
    assert bool(torch.isfinite(got).all())
    for i in range(R):
        assert torch.equal(_bits(got[i]), _bits(ref_logits[i])), (weights, R, i, float((got[i] - ref_logits[i]).abs().max()))
        assert torch.equal(_bits(spec.k_cache[:, :, P + i]), _bits(ref_k[i])), (weights, R, i, "K")
        assert torch.equal(_bits(spec.v_cache[:, :, P + i]), _bits(ref_v[i])), (weights, R, i, "V")
        assert torch.equal(_bits(spec.vt_cache[:, :, :, P + i]), _bits(ref_vt[i])), (weights, R, i, "V^T")
    assert bool(torch.isnan(spec.k_cache[:, :, P + R:].float()).all()), "a cache row at or behind P + R was written"
    # the tail: the selections are the argmax of every row; the accepted run follows the rule
    sel = got.argmax(-1).tolist()
    a = 0
    while a < R - 1 and sel[a] == rows[a + 1]:
        a += 1
    assert spec.generated().tolist() == sel[:a + 1]
    assert spec.stats() == {"steps": 1, "proposed": R - 1, "accepted": a, "emitted": a + 1}
    assert spec.cache_len == P + a + 1 and int(spec.d_rows[0].item()) == sel[a]


def test_the_proposer_kernel_is_propose_ngram():
    """teo_spec_propose against teochat_amd.speculative.propose_ngram on 200 seeded histories: lengths 1 .. 600, alphabets of 2 .. 6 ids
    (matches are common), image sentinels sprinkled in, rows 1 .. 16, n-grams up to 1 .. 4."""
    lib = G.lib()
    rng = random.Random(2024)
    hist_d = torch.zeros(640, dtype=torch.int64, device=DEV)
    len_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    rows_d = torch.zeros(16, dtype=torch.int64, device=DEV)
    nd_d = torch.zeros(1, dtype=torch.int32, device=DEV)
    with_drafts = 0
    for case in range(200):
        n = 1 + case * 599 // 189 if case < 190 else rng.randint(1, 12)         # 1 .. 600, then ten short ones
        alpha = list(range(10, 10 + rng.randint(2, 6)))
        h = [rng.choice(alpha) if rng.random() > 0.03 else -200 for _ in range(n)]
        if h[-1] < 0:
            h[-1] = alpha[0]                                                  # the last id is an emitted token
        R, nmax = rng.randint(1, 16), rng.randint(1, 4)
        hist_d.fill_(-7)
        hist_d[:n] = torch.tensor(h, dtype=torch.int64)
        len_d.fill_(n)
        rows_d.fill_(-1)
        rows_d[0] = h[-1]
        nd_d.fill_(-1)
        L.check(lib.teo_spec_propose(G.p(hist_d), G.p(len_d), G.p(rows_d), G.p(nd_d), R, nmax, G.stream()), "teo_spec_propose")
        want = propose_ngram(h, R, nmax)
        got_n, got = int(nd_d.item()), rows_d.tolist()
        assert got_n == len(want) and got[1:1 + got_n] == want, (case, h[-8:], R, nmax, want, got)
        assert got[0] == h[-1] and got[1 + got_n:R] == [h[-1]] * (R - 1 - got_n), (case, "unused rows hold the pending token")
        assert got[R:] == [-1] * (16 - R), (case, "rows behind R are not written")
        with_drafts += bool(want)
    assert with_drafts > 100


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_graph_replay_equals_plain_launches(sample):
    """The captured verify step replayed n times == n plain launches: tokens, position, stats and the sampler's draw counter; replays
    behind the stop change nothing."""
    from tests.test_model_gpu import build
    model, _ = build("tinyB", torch.float32)
    eng = model.engine
    V = eng.cfg.vocab_size
    base = O.synthetic_prompt_ids(12, 0, V, seed=5).tolist()
    ids = torch.tensor(base + base + base[:5])                               # a prompt that repeats itself: the proposer finds drafts
    emb = model.get_model().embed_tokens(ids.view(1, -1).to(DEV))[0]
    runs = []
    for use_graph in (True, False):
        spec = SpecDecoder(eng, 4, max_new=64)
        first = int(spec.prefill(emb)[0].argmax())
        spec.begin(first, ids.tolist() + [first], do_sample=sample, temperature=0.8, top_k=20, top_p=0.9, seed=1234, max_new=20)
        counts = [spec.steps(3, use_graph=use_graph) for _ in range(3)]
        spec.steps(14, use_graph=use_graph)                                   # 23 steps emit at least 23 > 20 tokens: runs into max_new
        assert spec.stopped() and int(spec.d_count.item()) == 20
        frozen = (spec.generated().tolist(), spec.cache_len, spec.stats(), spec.d_rng.tolist())
        spec.steps(2, use_graph=use_graph)
        assert frozen == (spec.generated().tolist(), spec.cache_len, spec.stats(), spec.d_rng.tolist())
        assert spec.cache_len == ids.numel() + 20 and (spec.d_rng.tolist()[1] == 21) == sample
        runs.append((counts,) + frozen)
    assert runs[0] == runs[1]
    assert runs[0][3]["steps"] <= 20
