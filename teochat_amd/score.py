"""Host-side planning for scoring the options of a closed-set question in one pass over the weights (include/teo_hip_score.h).

Every option is a short continuation ("branch") of one cached prompt of `past` rows.  Option c with tokens t_0 .. t_{n-1} FEEDS
t_0 .. t_{n-2}: the row that feeds t_k predicts t_{k+1}, and t_0 is predicted by the prompt's last row (the logits the prompt's own
prefill returned).  The fed rows of all options are packed behind each other; row i of a pass lands in cache row past + i, carries
the RoPE position past + i - branch_start[i] and sees the prompt and the rows of its own branch up to itself.
"""

PROMPT_ROW = -1          # `row` of a (row, label, option) triple whose logits are the prompt's last row


def plan_branches(option_ids, past, max_seq, max_rows):
    """option_ids: one non-empty list of token ids per option.  Returns a list of passes, each a dict with
         rows          token ids to feed, packed option by option
         branch_start  per row, the index of the first row of its option in this pass
         positions     per row, past + i - branch_start[i]
         triples       (row, label, option): logits row `row` of this pass (PROMPT_ROW: the prompt's last row) predicts token
                       `label` of option `option` -- exactly one triple per token of every option of the pass
         options       the options of the pass, in order
    Options keep their order and are never cut: a pass is closed when the next option would take it past max_rows rows or past
    max_seq cache rows.  Options that feed nothing (one token) ride along with whatever pass is open.  An option that does not fit
    into an empty pass raises ValueError."""
    past, max_seq, max_rows = int(past), int(max_seq), int(max_rows)
    if past < 1:
        raise ValueError("plan_branches: the prompt must hold at least one row (its last row predicts every option's first token)")
    cap = min(max_rows, max_seq - past)
    passes = []

    def new_pass():
        return dict(rows=[], branch_start=[], positions=[], triples=[], options=[])

    cur = new_pass()
    for c, ids in enumerate(option_ids):
        ids = [int(t) for t in ids]
        if not ids:
            raise ValueError(f"plan_branches: option {c} has no tokens")
        feed = len(ids) - 1
        if feed > cap:
            raise ValueError(f"plan_branches: option {c} feeds {feed} rows; at most {cap} fit (max_rows {max_rows}, max_seq {max_seq} - "
                             f"prompt {past})")
        if len(cur["rows"]) + feed > cap:
            passes.append(cur)
            cur = new_pass()
        start = len(cur["rows"])
        cur["options"].append(c)
        cur["triples"].append((PROMPT_ROW, ids[0], c))
        for k in range(feed):
            cur["rows"].append(ids[k])
            cur["branch_start"].append(start)
            cur["positions"].append(past + k)
            cur["triples"].append((start + k, ids[k + 1], c))
    if cur["options"]:
        passes.append(cur)
    return passes
