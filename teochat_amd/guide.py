"""Guided decoding, host side: finite automata over token ids (include/teo_hip_guide.h runs them inside the decode step's tail).

A `TokenGuide` is ONE table `next` (numpy uint16 [S][V]) and a start state: next[s][t] == NONE (0xFFFF) means token t is not allowed in
state s, any other value is the successor state.  There is no separate allow mask.  EOS is an ordinary token: every accepting state has
next[s][eos] = END, and END -- always the last state -- allows only EOS and loops on itself, so a conversation that runs on behind its
stop inside a chunk of graph replays stays well defined.  EOS remains the stop of generate(); the guide decides when EOS is allowed.
`max_new_tokens` may still cut an answer in the middle of the pattern.

Builders:
  TokenGuide.from_sequences(seqs, eos)         a trie: closed-set generation, token by token
  TokenGuide.from_regex(pattern, pieces, eos)  a regex subset, matched as a FULL match over the bytes the tokens spell
  pieces_of(tokenizer)                         `pieces` for ByteTokenizer and HF LLaMA (sentencepiece) tokenizers
  GuideSet(members)                            several guides in one table, one start state per member; None = "anything goes"

The regex subset is that of Python's `re` on BYTES patterns: literals, escapes (\\d \\s \\w \\D \\S \\W \\n \\t \\r \\f \\v \\xHH and any
escaped punctuation), classes [a-z0-9] and [^...], `.` (any byte but newline), groups `( )` / `(?: )`, `|`, and the quantifiers
* + ? {m} {m,} {m,n} (and their lazy forms, which match the same strings in full).  No anchors, back-references, look-around,
possessive or stacked quantifiers (`a*+`, `a**`): ValueError.  The DFA is not minimised and bounded repeats are unrolled, so nested
bounded repeats multiply: a pattern whose automaton would pass 65534 states raises ValueError ("... states exceed 65534").

Sentencepiece: LLaMA's tokenizer spells a word at the start of the answer, and after a space, with a leading "▁" (a space in `pieces`).
Whether the first generated token carries that space depends on the prompt's last token, so the rule is the CALLER's to put into the
pattern -- e.g. " ?" in front -- and not something from_regex guesses.
"""
import numpy as np

NONE = 0xFFFF
MAX_STATES = 65534

# strings the reference's two answer parsers accept: r"\[(\d+), (\d+), (\d+), (\d+)\]" (one box) and r"\[(.*?)\]" whose groups must split
# on "," into numbers (a list of boxes).  The digits are bounded: coordinates are percentages.
BOX_PATTERN = r"\[\d{1,3}, \d{1,3}, \d{1,3}, \d{1,3}\]"
BOX_LIST_PATTERN = BOX_PATTERN + r"(, " + BOX_PATTERN + r")*"


class TokenGuide:
    """transitions: one dict {token: successor} per state (states are 0 .. len - 1, without END); accepting: the states in which the
    answer may end; start: the first state.  The constructor
      - raises ValueError when a state reachable from `start` allows no token and is not accepting (a dead state), when a transition
        names `eos`, a token outside 0..vocab-1 or a state that does not exist, and when nothing can be accepted from `start`;
      - adds END and next[s][eos] = END for every accepting s;
      - prunes: states that cannot reach END disappear together with the transitions into them, and so do states `start` cannot reach;
      - renumbers the rest in breadth-first order from `start` (= state 0), END last; more than 65534 states: ValueError."""

    def __init__(self, transitions, accepting, start, vocab, eos):
        vocab, eos, start = int(vocab), int(eos), int(start)
        n = len(transitions)
        if not 0 <= eos < vocab:
            raise ValueError(f"eos {eos} outside 0..{vocab - 1}")
        if not 0 <= start < n:
            raise ValueError(f"start state {start} outside 0..{n - 1}")
        accepting = {int(s) for s in accepting}
        if any(not 0 <= s < n for s in accepting):
            raise ValueError("an accepting state does not exist")
        for s, row in enumerate(transitions):
            for t, q in row.items():
                if not 0 <= t < vocab or t == eos:
                    raise ValueError(f"state {s}: token {t} is EOS or outside 0..{vocab - 1}")
                if not 0 <= q < n:
                    raise ValueError(f"state {s}: successor {q} does not exist")
        # reachable dead states are an error of the caller's automaton, not something to prune silently
        seen, todo = {start}, [start]
        while todo:
            s = todo.pop()
            if not transitions[s] and s not in accepting:
                raise ValueError(f"state {s} is reachable, allows no token and is not accepting")
            for q in transitions[s].values():
                if q not in seen:
                    seen.add(q)
                    todo.append(q)
        # states that reach END: backwards from the accepting states
        back = [[] for _ in range(n)]
        for s, row in enumerate(transitions):
            for q in set(row.values()):
                back[q].append(s)
        live, todo = set(accepting), list(accepting)
        while todo:
            q = todo.pop()
            for s in back[q]:
                if s not in live:
                    live.add(s)
                    todo.append(s)
        if start not in live:
            raise ValueError("no accepting state can be reached from the start state")
        order, index = [start], {start: 0}
        for s in order:                                          # breadth first, over live states only
            for t in sorted(transitions[s]):
                q = transitions[s][t]
                if q in live and q not in index:
                    index[q] = len(order)
                    order.append(q)
        S = len(order) + 1
        if S > MAX_STATES:
            raise ValueError(f"{S} states exceed {MAX_STATES}")
        end = S - 1
        table = np.full((S, vocab), NONE, dtype=np.uint16)
        for s in order:
            row = table[index[s]]
            for t, q in transitions[s].items():
                if q in live:
                    row[t] = index[q]
            if s in accepting:
                row[eos] = end
        table[end, eos] = end
        self.next, self.start, self.end, self.eos = table, 0, end, eos
        self.n_states, self.vocab = S, vocab

    # ------------------------------------------------------------------ reading the table
    @property
    def table_bytes(self):
        return int(self.next.nbytes)

    def allowed(self, state):
        """the sorted token ids allowed in `state`"""
        return np.nonzero(self.next[state] != NONE)[0].tolist()

    def step(self, state, token):
        """the successor state, or None when `token` is not allowed in `state`"""
        q = int(self.next[state, token])
        return None if q == NONE else q

    def is_accepting(self, state):
        return int(self.next[state, self.eos]) == self.end

    def walk(self, tokens, state=None):
        """the state after `tokens` from `state` (default: start), or None when one of them is not allowed"""
        s = self.start if state is None else int(state)
        for t in tokens:
            s = self.step(s, int(t))
            if s is None:
                return None
        return s

    def accepts(self, tokens):
        """`tokens` (without EOS) followed by EOS is a walk from start to END"""
        s = self.walk(tokens)
        return s is not None and s != self.end and self.is_accepting(s)

    # ------------------------------------------------------------------ builders
    @classmethod
    def universal(cls, vocab, eos):
        """one state that allows every token (EOS included) and loops on itself: the plain decode loop"""
        g = cls.__new__(cls)
        g.next = np.zeros((1, int(vocab)), dtype=np.uint16)
        g.start, g.end, g.eos, g.n_states, g.vocab = 0, 0, int(eos), 1, int(vocab)
        return g

    @classmethod
    def from_sequences(cls, sequences, eos, vocab=None):
        """A trie over the id lists: exactly these sequences, each followed by EOS.  vocab: the table's width (the model's vocabulary);
        left out, the largest id + 1."""
        seqs = [[int(t) for t in s] for s in sequences]
        if not seqs or any(not s for s in seqs):
            raise ValueError("from_sequences: at least one sequence, none of them empty")
        if vocab is None:
            vocab = max(max(max(s) for s in seqs), int(eos)) + 1
        trans, accepting = [{}], set()
        for s in seqs:
            cur = 0
            for t in s:
                if t not in trans[cur]:
                    trans.append({})
                    trans[cur][t] = len(trans) - 1
                cur = trans[cur][t]
            accepting.add(cur)
        return cls(trans, accepting, 0, vocab, eos)

    @classmethod
    def from_regex(cls, pattern, pieces, eos):
        """pattern: str or bytes in the subset of the module docstring, matched as a full match.  pieces[t]: the bytes token t contributes,
        or None for a token that is never allowed (BOS, pad, <unk>, image sentinels; an empty piece counts as None).  Stages: Thompson NFA,
        subset DFA over bytes, prune, lift to tokens by walking a trie of the pieces through the DFA once per state."""
        dfa, accepting = _byte_dfa(pattern)
        vocab = len(pieces)
        root = [{}, []]                                          # [children by byte, tokens that end here]
        for t, p in enumerate(pieces):
            if p is None or len(p) == 0 or t == int(eos):
                continue
            node = root
            for b in bytes(p):
                node = node[0].setdefault(b, [{}, []])
            node[1].append(t)
        trans = []
        for s in range(len(dfa)):
            row = {}
            stack = [(root, s)]
            while stack:
                node, q = stack.pop()
                for t in node[1]:
                    row[t] = q
                dq = dfa[q]
                for b, child in node[0].items():
                    nq = dq.get(b)
                    if nq is not None:
                        stack.append((child, nq))
            trans.append(row)
        trans, accepting, start = _prune(trans, accepting, 0)
        if start is None:
            raise ValueError(f"from_regex: this vocabulary cannot spell any string of {pattern!r}")
        return cls(trans, accepting, start, vocab, eos)


def _prune(trans, accepting, start):
    """drop the states that cannot reach an accepting state and the transitions into them; (trans, accepting, start) renumbered, start
    None when nothing is left"""
    n = len(trans)
    back = [[] for _ in range(n)]
    for s, row in enumerate(trans):
        for q in set(row.values()):
            back[q].append(s)
    live, todo = set(accepting), list(accepting)
    while todo:
        q = todo.pop()
        for s in back[q]:
            if s not in live:
                live.add(s)
                todo.append(s)
    if start not in live:
        return [], set(), None
    keep = sorted(live)
    index = {s: i for i, s in enumerate(keep)}
    out = [{t: index[q] for t, q in trans[s].items() if q in live} for s in keep]
    return out, {index[s] for s in accepting}, index[start]


class GuideSet:
    """Several guides in one table: member i's states sit at offsets[i] .., its start state is starts[i].  A None member is the one-state
    automaton that allows everything (it needs `vocab`).  Members that are the same object share their rows."""

    def __init__(self, members, vocab=None, eos=None):
        members = list(members)
        real = [m for m in members if m is not None]
        if vocab is None:
            if not real:
                raise ValueError("GuideSet: only None members: give the vocabulary size")
            vocab = real[0].vocab
        vocab = int(vocab)
        if any(m.vocab != vocab for m in real):
            raise ValueError("GuideSet: the members' tables differ in width")
        blocks, off, at = [], 0, {}
        self.starts, self.offsets = [], []
        for m in members:
            key = id(m) if m is not None else None
            if key not in at:
                tab = m.next if m is not None else np.zeros((1, vocab), dtype=np.uint16)
                at[key] = (off, m.start if m is not None else 0)
                blocks.append(np.where(tab == NONE, NONE, tab.astype(np.uint32) + off).astype(np.uint16))
                off += tab.shape[0]
                if off > MAX_STATES:
                    raise ValueError(f"GuideSet: {off} states exceed {MAX_STATES}")
            self.offsets.append(at[key][0])
            self.starts.append(at[key][0] + at[key][1])
        self.members = members
        self.next = np.concatenate(blocks, axis=0)
        self.n_states, self.vocab = off, vocab
        self.eos = eos if eos is not None else (real[0].eos if real else None)

    @property
    def table_bytes(self):
        return int(self.next.nbytes)


def pieces_of(tokenizer, vocab=None):
    """pieces[t] = the bytes token t contributes to the decoded text, or None for a token a guide must never allow.
    vocab: the MODEL's vocabulary size (config.vocab_size) when it is larger than the tokenizer's -- embedding rows no token maps to
    (padding of the matrix, added image tokens) are None; a guide's table must be as wide as the model's logits.
    ByteTokenizer: 3 + b -> bytes([b]), ids 0..2 None.  HF LLaMA tokenizers (convert_ids_to_tokens): "▁" -> a space, "<0xHH>" -> that
    byte, special tokens (all_special_ids, and anything of the form <...> that is no byte token) None."""
    from .tokenizer_stub import ByteTokenizer
    if isinstance(tokenizer, ByteTokenizer):
        return _padded([None, None, None] + [bytes([b]) for b in range(256)], vocab)
    n = len(tokenizer)
    special = set(getattr(tokenizer, "all_special_ids", None) or [])
    out = []
    for t, tok in enumerate(tokenizer.convert_ids_to_tokens(list(range(n)))):
        if t in special or tok is None:
            out.append(None)
        elif len(tok) == 6 and tok.startswith("<0x") and tok.endswith(">"):
            out.append(bytes([int(tok[3:5], 16)]))
        elif tok.startswith("<") and tok.endswith(">") and len(tok) > 2:
            out.append(None)
        else:
            out.append(tok.replace("▁", " ").encode("utf-8"))
    return _padded(out, vocab)


def _padded(pieces, vocab):
    if vocab is not None and int(vocab) < len(pieces):
        raise ValueError(f"the tokenizer has {len(pieces)} tokens, the model's vocabulary only {vocab}")
    return pieces + [None] * (int(vocab) - len(pieces) if vocab is not None else 0)


def named_guide(name, tokenizer, vocab=None):
    """The guides the eval driver knows by name.  "boxes": BOX_LIST_PATTERN over the tokenizer's pieces; for a sentencepiece tokenizer
    an optional leading space is allowed in front (the caller's rule, see the module docstring)."""
    from .tokenizer_stub import ByteTokenizer
    if name != "boxes":
        raise ValueError(f"unknown guide {name!r} (known: 'boxes')")
    lead = "" if isinstance(tokenizer, ByteTokenizer) else " ?"
    return TokenGuide.from_regex(lead + BOX_LIST_PATTERN, pieces_of(tokenizer, vocab), int(tokenizer.eos_token_id))


# ---------------------------------------------------------------------------------------------------------------- regex -> byte DFA
_ALL = (1 << 256) - 1
_DIGIT = sum(1 << b for b in range(48, 58))
_SPACE = sum(1 << b for b in b" \t\n\r\f\v")
_WORD = _DIGIT | sum(1 << b for b in range(65, 91)) | sum(1 << b for b in range(97, 123)) | (1 << 95)
_CLASS_ESC = {"d": _DIGIT, "D": _ALL ^ _DIGIT, "s": _SPACE, "S": _ALL ^ _SPACE, "w": _WORD, "W": _ALL ^ _WORD}
_CHAR_ESC = {"n": 10, "t": 9, "r": 13, "f": 12, "v": 11, "a": 7, "0": 0}
_MAX_REPEAT = 1000


class _Parser:
    """pattern bytes -> AST: ("set", mask) | ("cat", [..]) | ("alt", [..]) | ("rep", node, m, n or None)"""

    def __init__(self, pattern):
        self.p = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        self.i = 0

    def fail(self, what):
        raise ValueError(f"regex {self.p!r}: {what} at offset {self.i}")

    def peek(self):
        return self.p[self.i:self.i + 1].decode("latin-1") if self.i < len(self.p) else ""

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        arms = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            arms.append(self.cat())
        return arms[0] if len(arms) == 1 else ("alt", arms)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        while True:
            c = self.peek()
            if c == "*":
                m, n = 0, None
            elif c == "+":
                m, n = 1, None
            elif c == "?":
                m, n = 0, 1
            elif c == "{":
                j = self.p.find(b"}", self.i)
                body = self.p[self.i + 1:j].decode("latin-1") if j > 0 else ""
                parts = body.split(",")
                if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
                    self.fail("malformed {m,n}")
                m = int(parts[0])
                n = m if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
                if (n is not None and n < m) or max(m, n or 0) > _MAX_REPEAT:
                    self.fail("bad repeat bounds")
                self.i = j
            else:
                return node
            self.i += 1
            if self.peek() == "?":                               # a lazy quantifier: the same language under a full match
                self.i += 1
            if self.peek() in ("*", "+", "?", "{"):              # a** is an error in `re`, a*+ a possessive quantifier: neither is taken
                self.fail("multiple repeat")
            return ("rep", node, m, n)

    def escape(self, in_class):
        """after a backslash: ("set", mask) for a class escape, or a byte value"""
        c = self.peek()
        if c == "":
            self.fail("trailing backslash")
        self.i += 1
        if c in _CLASS_ESC:
            return ("set", _CLASS_ESC[c])
        if c == "x":
            h = self.p[self.i:self.i + 2].decode("latin-1")
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF" for ch in h):
                self.fail("malformed \\xHH")
            self.i += 2
            return int(h, 16)
        if c in _CHAR_ESC:
            return _CHAR_ESC[c]
        if c == "b" and in_class:
            return 8
        if c.isalnum():
            self.fail(f"unsupported escape \\{c}")
        return ord(c)

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == "(":
            if self.p[self.i:self.i + 2] == b"?:":
                self.i += 2
            elif self.peek() == "?":
                self.fail("unsupported group (?...)")
            node = self.alt()
            if self.peek() != ")":
                self.fail("missing ')'")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            return ("set", _ALL ^ (1 << 10))
        if c == "\\":
            e = self.escape(False)
            return e if isinstance(e, tuple) else ("set", 1 << e)
        if c in "*+?{":
            self.fail("nothing to repeat")
        if c in "^$":
            self.fail("anchors are not supported (the pattern is a full match already)")
        return ("set", 1 << ord(c))

    def char_class(self):
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        mask, first = 0, True
        while True:
            c = self.peek()
            if c == "":
                self.fail("missing ']'")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            lo = self.escape(True) if c == "\\" else ord(c)
            if isinstance(lo, tuple):
                mask |= lo[1]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in (b"]", b""):
                self.i += 1
                d = self.peek()
                self.i += 1
                hi = self.escape(True) if d == "\\" else ord(d)
                if isinstance(hi, tuple) or hi < lo:
                    self.fail("bad character range")
                for b in range(lo, hi + 1):
                    mask |= 1 << b
            else:
                mask |= 1 << lo
        return ("set", (_ALL ^ mask) if neg else mask)


def _thompson(ast):
    """AST -> (eps, arcs, start, accept): eps[s] = list of states, arcs[s] = list of (mask, target)"""
    eps, arcs = [], []

    def new():
        eps.append([])
        arcs.append([])
        return len(eps) - 1

    def build(node):
        kind = node[0]
        if kind == "set":
            a, b = new(), new()
            arcs[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = new()
            for item in node[1]:
                x, y = build(item)
                eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = new(), new()
            for arm in node[1]:
                x, y = build(arm)
                eps[a].append(x)
                eps[y].append(b)
            return a, b
        _, inner, m, n = node
        a = b = new()
        for _ in range(m):
            x, y = build(inner)
            eps[b].append(x)
            b = y
        if n is None:                                            # inner*
            x, y = build(inner)
            loop, out = new(), new()
            eps[b].append(loop)
            eps[loop] += [x, out]
            eps[y].append(loop)
            return a, out
        out = new()
        for _ in range(n - m):                                   # (inner (inner ...)?)?
            eps[b].append(out)
            x, y = build(inner)
            eps[b].append(x)
            b = y
        eps[b].append(out)
        return a, out

    start, accept = build(ast)
    return eps, arcs, start, accept


def _byte_dfa(pattern):
    """(dfa, accepting): dfa[s] = {byte: successor}, start state 0, every state able to reach an accepting one"""
    eps, arcs, start, accept = _thompson(_Parser(pattern).parse())

    def closure(states):
        out, todo = set(states), list(states)
        while todo:
            for q in eps[todo.pop()]:
                if q not in out:
                    out.add(q)
                    todo.append(q)
        return frozenset(out)

    s0 = closure([start])
    index, order, dfa = {s0: 0}, [s0], []
    for cur in order:
        moves = [(mask, q) for s in cur for mask, q in arcs[s]]
        row, cache = {}, {}
        for b in range(256):
            bit = 1 << b
            key = frozenset(q for mask, q in moves if mask & bit)
            if not key:
                continue
            if key not in cache:
                nxt = closure(key)
                if nxt not in index:
                    index[nxt] = len(order)
                    order.append(nxt)
                    if len(order) > 4 * MAX_STATES:
                        raise ValueError("regex: the byte DFA has too many states")
                cache[key] = index[nxt]
            row[b] = cache[key]
        dfa.append(row)
    accepting = {i for i, st in enumerate(order) if accept in st}
    dfa, accepting, start = _prune(dfa, accepting, 0)
    if start is None:
        raise ValueError(f"regex {pattern!r} matches nothing")
    if start != 0:                                               # _prune keeps the order, so a live start stays state 0
        raise AssertionError("pruning moved the start state")
    return dfa, accepting
