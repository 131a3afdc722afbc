"""Beam search for one conversation inside the device decode loop (include/teo_hip_beam.h): generate(num_beams=B).

The B running beams are the B slots of the model's StreamDecoder -- its caches, workspace and descriptors; nothing of those is allocated
twice.  The prompt is prefilled into slot 0, the first selection runs on the prefill row, teo_kv_fork copies the prompt rows into the
other slots (which the share table then reads once per step for all beams), and the beam step -- layers, selection, reorder of the KV
tails, embedding of the new tokens -- is replayed from a hipGraph in chunks; the host looks at d_done once per chunk and backtracks the
finished hypotheses through the (token, parent) history when the search has ended.

  check_beam_args  the keywords' refusals
  len_norm_table   fp32(float64(n) ** length_penalty): the device divides, it never calls pow
  BeamDecoder      the device state on top of a StreamDecoder, begin / steps / finish
"""
import ctypes as C

import torch

from . import _lib as L
from .decode_host import StepGraphs, _p

EARLY = {False: 0, True: 1, "never": 2}


class BeamOutput(dict):
    """generate(num_beams=B, return_dict_in_generate=True): `sequences` int64 [n, prompt + longest], `sequences_scores` fp32 [n] (the
    accumulated log-probability divided by length ** length_penalty), best first"""

    def __init__(self, sequences=None, sequences_scores=None):
        super().__init__(sequences=sequences, sequences_scores=sequences_scores)
        self.sequences, self.sequences_scores = sequences, sequences_scores


def check_beam_args(num_beams, num_return_sequences=None, length_penalty=None, early_stopping=None, do_sample=False):
    """The beam keywords of generate() as (num_beams, num_return_sequences, length_penalty, early_stopping 0 / 1 / 2), or None when
    the search is off (num_beams None or 1).  ValueError, with a sentence, for what include/teo_hip_beam.h cannot hold."""
    B = 1 if num_beams is None else int(num_beams)
    n = 1 if num_return_sequences is None else int(num_return_sequences)
    if not 1 <= B <= L.MAX_DECODE_BATCH:
        raise ValueError(f"num_beams {num_beams} outside 1..{L.MAX_DECODE_BATCH} (one beam per slot of the batched decode step)")
    if not 1 <= n <= B:
        raise ValueError(f"num_return_sequences {n} outside 1..num_beams {B}")
    if B == 1:
        return None
    if do_sample:
        raise ValueError("do_sample=True with num_beams > 1: beam sampling is not built (greedy beam search only)")
    if early_stopping is None:
        early_stopping = False
    if isinstance(early_stopping, str):
        if early_stopping != "never":
            raise ValueError(f"early_stopping {early_stopping!r}: False, True or \"never\"")
    else:
        early_stopping = bool(early_stopping)
    lp = 1.0 if length_penalty is None else float(length_penalty)
    if lp != lp or lp in (float("inf"), float("-inf")):
        raise ValueError(f"length_penalty {length_penalty} must be a finite number")
    return B, n, lp, EARLY[early_stopping]


def len_norm_table(max_new, length_penalty):
    """fp32 [max_new + 1]: [n] = fp32(float64(n) ** length_penalty); [0] is unused"""
    t = torch.tensor([1.0] + [float(n) ** float(length_penalty) for n in range(1, int(max_new) + 1)], dtype=torch.float64).to(torch.float32)
    if not bool(torch.isfinite(t).all()) or bool((t <= 0).any()):
        raise ValueError(f"length_penalty {length_penalty} leaves fp32 at {max_new} tokens")
    return t


def backtrack(hist_token, hist_parent, step, parent, token):
    """the tokens of the hypothesis that ended at `step` with `token` behind running beam `parent` of step - 1"""
    out, b = [int(token)], int(parent)
    for s in range(int(step) - 1, -1, -1):
        out.append(int(hist_token[s][b]))
        b = int(hist_parent[s][b])
    return out[::-1]


class BeamDecoder(StepGraphs):
    """The beam state over `dec` (a StreamDecoder: one slot per beam) for answers of up to `max_new` tokens."""

    def __init__(self, dec, max_new):
        self.dec, self.eng, self.lib, self.B = dec, dec.eng, dec.lib, dec.B
        if not 2 <= self.B <= L.MAX_DECODE_BATCH:
            raise ValueError(f"num_beams {self.B} outside 2..{L.MAX_DECODE_BATCH}")
        self.cap = int(max_new)
        B, dev, bd = self.B, dec.eng.device, dec.bd
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.d_len_norm = torch.ones(self.cap + 1, dtype=f32, device=dev)
        self.d_scores = torch.zeros(B, dtype=f32, device=dev)
        self.d_parent = torch.zeros(B, dtype=i32, device=dev)
        self.d_hist_token = torch.zeros(self.cap, B, dtype=i64, device=dev)
        self.d_hist_parent = torch.zeros(self.cap, B, dtype=i32, device=dev)
        self.d_fin_score = torch.zeros(B, dtype=f32, device=dev)
        self.d_fin_step = torch.zeros(B, dtype=i32, device=dev)
        self.d_fin_parent = torch.zeros(B, dtype=i32, device=dev)
        self.d_fin_token = torch.zeros(B, dtype=i64, device=dev)
        self.d_flags = torch.zeros(3, dtype=i32, device=dev)          # fin_count, step, done
        self.d_cand_score = torch.zeros(B, 2 * B, dtype=f32, device=dev)
        self.d_cand_token = torch.zeros(B, 2 * B, dtype=i32, device=dev)
        self.d_best_score = torch.zeros(2 * B, dtype=f32, device=dev)
        self.d_best_flat = torch.zeros(2 * B, dtype=i64, device=dev)
        s = L.BeamState()
        s.num_beams, s.max_new, s.eos, s.early_stopping, s.length_penalty = B, 1, -1, 0, 1.0
        for name in ("d_len_norm", "d_scores", "d_parent", "d_hist_token", "d_hist_parent", "d_fin_score", "d_fin_step", "d_fin_parent",
                     "d_fin_token", "d_cand_score", "d_cand_token", "d_best_score", "d_best_flat"):
            setattr(s, name, getattr(self, name).data_ptr())
        s.d_token, s.d_pos = bd.d_token.data_ptr(), bd.d_pos.data_ptr()
        s.d_fin_count, s.d_step, s.d_done = (self.d_flags.data_ptr() + 4 * i for i in range(3))
        self.state = s
        self.prompt_rows = 0
        StepGraphs.__init__(self)
        self.eng.on_tune(self, BeamDecoder._drop_graph)
        self.eng.on_options(self, lambda o, _desc: o._drop_graph())

    # ------------------------------------------------------------------ begin
    def begin(self, embeds, eos=None, max_new=20, length_penalty=1.0, early_stopping=0):
        """Prefill embeds [S, D] into slot 0, select the first B beams on the prefill row, fork the prompt rows into the other slots
        and arm every slot.  Returns the prefill logits [1, V] (fp32, device)."""
        dec, bd, B, s = self.dec, self.dec.bd, self.B, self.state
        max_new = int(max_new)
        if not 1 <= max_new <= self.cap:
            raise ValueError(f"max_new_tokens {max_new} outside 1..{self.cap}")
        P = int(embeds.shape[0])
        if P + max_new > self.eng.max_seq:
            raise ValueError(f"prompt ({P}) + max_new_tokens ({max_new}) exceeds max_seq {self.eng.max_seq}")
        V = int(self.eng.cfg.vocab_size)
        eos = -1 if eos is None else int(eos)
        if not -1 <= eos < V:
            raise ValueError(f"eos_token_id {eos} outside the vocabulary 0..{V - 1}")
        norm = len_norm_table(max_new, length_penalty)
        s.max_new, s.eos, s.early_stopping, s.length_penalty = max_new, eos, int(early_stopping), float(length_penalty)
        dec.reset()
        dec.configure()                              # greedy, no device stop ids: the selection decides the end
        logits = dec.refill([0], [embeds]).contiguous()
        with self.eng.phase() as st:
            self.d_len_norm[:max_new + 1].copy_(norm)
            self.d_scores.zero_()
            self.d_fin_score.fill_(float("-inf"))
            self.d_flags.zero_()
            bd.d_pos.fill_(P - 1)                    # the first selection advances every slot to the first new token's position
            L.check(self.lib.teo_beam_select(_p(logits), V, 1, V, C.byref(s), st), "teo_beam_select")
        dec.held[0] = ("beam", (), (), P)            # slot 0's prefill wrote P rows: what fork() checks
        dec.fork(0, list(range(1, B)), P)
        ws = dec._workspace()
        with self.eng.phase() as st:
            dec.d_share_lead.copy_(torch.tensor(dec.share.lead, dtype=torch.int32))
            dec.d_share_rows.copy_(torch.tensor(dec.share.rows, dtype=torch.int32))
            dec.share.dirty = False
            for slot in range(B):
                L.check(self.lib.teo_llama_decode_stream_arm(C.byref(bd.desc), C.byref(dec.state), slot, _p(ws), ws.numel(), st),
                        "teo_llama_decode_stream_arm")
        self.prompt_rows = P
        return logits

    # ------------------------------------------------------------------ step
    def graph_key(self):
        """what the captured beam step holds by value beyond the decoder's fixed addresses"""
        s = self.state
        return (self.dec._workspace().data_ptr(), self.prompt_rows, s.max_new, s.eos, s.early_stopping, s.length_penalty)

    def steps(self, n, use_graph=True):
        """n beam steps; behind the end of the search they change nothing"""
        dec, bd = self.dec, self.dec.bd
        ws = dec._workspace()
        d, s_, sh_, b_, P = C.byref(bd.desc), C.byref(dec.state), C.byref(dec._share), C.byref(self.state), self.prompt_rows
        with self.eng.phase() as st:
            self.replay_or_step(self.eng.stream, self.graph_key(), int(n), use_graph,
                                lambda out: L.check(self.lib.teo_llama_decode_beam_graph_create(d, s_, sh_, b_, P, _p(ws), ws.numel(), st, out),
                                                    "teo_llama_decode_beam_graph_create"),
                                lambda: L.check(self.lib.teo_llama_decode_beam_step(d, s_, sh_, b_, P, _p(ws), ws.numel(), st),
                                                "teo_llama_decode_beam_step"))

    def flags(self):
        """(finished hypotheses, selections done, done) -- one small copy"""
        with self.eng.phase():
            return tuple(int(x) for x in self.d_flags.tolist())

    def run(self, chunk=16):
        """replay in chunks until the search has ended; returns the number of selections"""
        chunk = max(int(chunk), 1)
        fin, step, done = self.flags()
        while not done and step < self.state.max_new:
            self.steps(min(chunk, self.state.max_new - step))
            fin, step, done = self.flags()
        if not done:
            raise RuntimeError(f"beam search did not end within max_new_tokens {self.state.max_new} selections")
        return step

    # ------------------------------------------------------------------ finish
    def finish(self, num_return_sequences=1):
        """[(score, tokens)] of the best finished hypotheses, best first, and {beam_steps, finished, reorder_rows}"""
        B = self.B
        with self.eng.phase():
            fin, step, _ = (int(x) for x in self.d_flags.tolist())
            f_score, f_step = self.d_fin_score.cpu(), self.d_fin_step.tolist()
            f_par, f_tok = self.d_fin_parent.tolist(), self.d_fin_token.tolist()
            h_tok, h_par = self.d_hist_token[:step].tolist(), self.d_hist_parent[:step].tolist()
        hyps = [(f_score[i].clone(), backtrack(h_tok, h_par, f_step[i], f_par[i], f_tok[i])) for i in range(min(fin, int(num_return_sequences)))]
        # selection s >= 1 ran inside a beam step and moved the s tail rows of every slot that changed parent; the last one ended the search
        # and moved nothing
        moved = sum(s * sum(1 for j in range(B) if h_par[s][j] != j) for s in range(1, step - 1))
        return hyps, dict(beam_steps=step, finished=fin, reorder_rows=moved)

    def end(self):
        """hand the slots back: every slot parked and free, the share table reset"""
        self.dec.reset()
