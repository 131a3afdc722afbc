"""Beam search for batch 1 restated in numpy (include/teo_hip_beam.h), for tests/test_beam_host.py (which holds this form to
`transformers`' _beam_search bit for bit) and tests/test_beam_gpu.py (which holds the kernels to this form bit for bit).  A plain helper
module (not a conftest).

Where `transformers` leaves an order open -- torch.topk on equal scores -- the order here is: key descending, then flat index b * V + v
ascending; finished hypotheses of equal score: old entries first, then rank order."""
import numpy as np

F32 = np.float32
NINF = F32(-np.inf)
EARLY = {False: 0, True: 1, "never": 2}


def len_norm_table(max_new, length_penalty):
    """[max_new + 1] fp32: [n] = fp32(float64(n) ** length_penalty); [0] is unused (1)"""
    return np.array([1.0] + [float(n) ** float(length_penalty) for n in range(1, int(max_new) + 1)], dtype=np.float64).astype(F32)


def new_state(B):
    """the search state before the first step: running scores, the finished set (score, step, parent, token), best first"""
    return dict(scores=np.full(B, NINF, F32), fin=[], step=0, done=False)


def beam_step(lp, state, *, B, eos, max_new, len_norm, early_stopping=False, length_penalty=1.0):
    """One selection.  lp: fp32 [n_rows, V] log-probabilities (n_rows = 1: the first step, row 0 only; else B), NaN read as -inf.
    Returns (candidates, running, state'): candidates = the 2B best [(key, beam, token)] in rank order (fewer when fewer keys are
    finite); running = (tokens [B], parents [B], scores [B]) of the next running beams; state' the updated state (with `done`)."""
    lp = np.asarray(lp, dtype=F32)
    n_rows, V = lp.shape
    assert n_rows in (1, B) and not state["done"]
    t = state["step"]
    n = t + 1
    run = np.zeros(1, F32) if n_rows == 1 else state["scores"]
    with np.errstate(all="ignore"):
        lp = np.where(np.isnan(lp), NINF, lp)
        keys = np.where(lp > NINF, (run[:, None] + lp).astype(F32), NINF).reshape(-1)
        keys = np.where(np.isnan(keys), NINF, keys)
    order = np.argsort(-keys, kind="stable")[:2 * B]                    # key descending, flat index ascending
    cands = [(F32(keys[i]), int(i) // V, int(i) % V) for i in order if keys[i] > NINF]
    toks, pars, scs = [], [], []
    fin = list(state["fin"])
    all_stop = True
    for rank, (key, b, v) in enumerate(cands):
        stop = v == eos or n >= max_new
        if not stop:
            all_stop = False
            if len(toks) < B:
                toks.append(v); pars.append(b); scs.append(key)
        elif rank < B:
            with np.errstate(all="ignore"):
                norm = F32(key / len_norm[n])
            if np.isnan(norm):
                norm = NINF
            at = 0
            while at < len(fin) and not fin[at][0] < norm:
                at += 1
            fin.insert(at, (norm, t, b, v))
            fin = fin[:B]
    for j in range(len(toks), B):
        toks.append(0); pars.append(j); scs.append(NINF)
    scores = np.array(scs, dtype=F32)
    done = all_stop
    if len(fin) == B:
        L = max_new if (EARLY[early_stopping] == 2 and length_penalty > 0.0) else n
        with np.errstate(all="ignore"):
            possible = F32(scores[0] / len_norm[L])
        if EARLY[early_stopping] == 1 or not possible > fin[B - 1][0]:
            done = True
    top = np.sort(keys)[::-1][:2 * B + 1]                               # for the tests' tie conditions: the 2B + 1 best keys
    new = dict(scores=scores, fin=fin, step=n, done=done, top_keys=top)
    return cands, (np.array(toks, np.int64), np.array(pars, np.int32), scores), new


def backtrack(hist_token, hist_parent, step, parent, token):
    """the tokens of a hypothesis that ended at `step` with `token` behind running beam `parent` of step - 1"""
    out = [int(token)]
    b = int(parent)
    for s in range(int(step) - 1, -1, -1):
        out.append(int(hist_token[s][b]))
        b = int(hist_parent[s][b])
    return out[::-1]


def beam_search(logprob_fn, *, B, eos, max_new, length_penalty=1.0, early_stopping=False, num_return_sequences=1, pad=None, on_step=None):
    """The loop.  logprob_fn(seqs) -> fp32 [len(seqs), V] log-probabilities of the next token behind each generated-token list in
    `seqs` ([[]] at the first step).  Returns (sequences [n_ret, longest] int64 padded with `pad`, else eos, else -1; scores [n_ret] fp32;
    the number of steps).  on_step(state) behind every step, for the tests' tie and gap conditions."""
    eos_ = -1 if eos is None else int(eos)
    ln = len_norm_table(max_new, length_penalty)
    st = new_state(B)
    hist_t, hist_p = [], []
    seqs = [[]]
    while not st["done"]:
        lp = np.asarray(logprob_fn(seqs), dtype=F32)
        cands, (toks, pars, _), st = beam_step(lp, st, B=B, eos=eos_, max_new=max_new, len_norm=ln, early_stopping=early_stopping,
                                               length_penalty=length_penalty)
        if on_step is not None:
            on_step(st)
        hist_t.append(toks); hist_p.append(pars)
        seqs = [backtrack(hist_t, hist_p, st["step"] - 1, pars[j], toks[j]) for j in range(B)]
    hyps = [(s, backtrack(hist_t, hist_p, step, par, tok)) for s, step, par, tok in st["fin"][:num_return_sequences]]
    fill = (pad or eos_) if eos_ >= 0 else -1                           # HF's fill rule, as written there: (pad or eos) if eos else -1
    longest = max(len(h) for _, h in hyps)
    out = np.full((len(hyps), longest), fill, np.int64)
    for i, (_, h) in enumerate(hyps):
        out[i, :len(h)] = h
    return out, np.array([s for s, _ in hyps], dtype=F32), st["step"]
