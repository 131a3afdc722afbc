"""Confidence figures from the token log-probabilities generate(logprobs=True) returns (include/teo_hip_logprob.h).

  answer_confidence   exp(mean log-probability) over the generated tokens, the stop token included: the geometric mean of the
                      per-token probabilities -- the calibration signal of a short classification answer
  box_confidences     the same mean over the tokens that spell each [x1, y1, x2, y2] of a detection answer: a per-box score that can be
                      thresholded or ranked
  confidence_record   both, with the raw values, for one answer (what the inference drivers attach to a record)

Under a guide the values are probabilities among the tokens the automaton allowed (token log-probabilities).  Host code only:
nothing here touches the device.
"""
import math

from .inference import _BBOX


def _floats(logprobs):
    return [float(v) for v in (logprobs.reshape(-1).tolist() if hasattr(logprobs, "reshape") else logprobs)]


def answer_confidence(logprobs):
    """exp(mean) of the log-probabilities (a sequence or a tensor; NaN entries -- behind a row's end -- are left out); 0.0 for none"""
    lp = [v for v in _floats(logprobs) if not math.isnan(v)]
    return math.exp(sum(lp) / len(lp)) if lp else 0.0


def box_confidences(pieces, new_ids, logprobs):
    """[(box [x1, y1, x2, y2], exp(mean logprob))] for every box inference.extract_bboxes finds in the decoded answer, in its order.
    pieces: guide.pieces_of(tokenizer) -- the bytes each token id contributes; new_ids / logprobs: the generated ids and their values.
    A box's tokens are those whose piece overlaps the substring from its opening `[` to its closing `]`; each token counts once per
    box.  A box the answer does not complete (cut off by max_new_tokens) does not match and is not reported."""
    ids = [int(t) for t in (new_ids.reshape(-1).tolist() if hasattr(new_ids, "reshape") else new_ids)]
    lp = _floats(logprobs)
    if len(lp) < len(ids):
        raise ValueError(f"box_confidences: {len(ids)} ids, {len(lp)} log-probabilities")
    spans, at = [], 0
    for t in ids:
        n = len(pieces[t] or b"") if 0 <= t < len(pieces) else 0
        spans.append((at, at + n))
        at += n
    text = b"".join(pieces[t] or b"" for t in ids if 0 <= t < len(pieces)).decode("latin-1")      # one character per byte: offsets are byte offsets
    out = []
    for m in _BBOX.finditer(text):
        lo, hi = m.span()
        inside = [lp[i] for i, (a, b) in enumerate(spans) if a < hi and b > lo and not math.isnan(lp[i])]
        out.append(([int(v) for v in m.groups()], math.exp(sum(inside) / len(inside)) if inside else 0.0))
    return out


def confidence_record(pieces, new_ids, logprobs):
    """{"logprobs": [...], "confidence": float, "box_confidences": [[box, score], ...]} of one answer (JSON-ready)"""
    lp = _floats(logprobs)
    return {"logprobs": lp, "confidence": answer_confidence(lp), "box_confidences": [[b, c] for b, c in box_confidences(pieces, new_ids, lp)]}
