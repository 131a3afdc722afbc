"""Guided decoding, host side (teochat_amd/guide.py; no GPU): the regex compiler against Python's `re`, the token lift against a
byte-by-byte walk, the trie, GuideSet, the constructor's checks, the fourth header's containment table and the wiring of `guide`
through run_inference* and the eval switch."""
import os
import random
import re

import numpy as np
import pytest
import torch

from teochat_amd import _lib as L
from teochat_amd import guide as GD
from teochat_amd import inference as I
from teochat_amd.tokenizer_stub import ByteTokenizer
from tests.test_containment_table import ROOT, arena, declared_functions, problems, reason

EOS = 2
BYTES = GD.pieces_of(ByteTokenizer())


def ids(text):
    return [3 + b for b in text.encode()]


def spell(tokens, pieces=BYTES):
    return b"".join(pieces[t] for t in tokens)


# pattern -> (strings that match, near misses)
PATTERNS = {
    GD.BOX_PATTERN: (["[1, 2, 3, 4]", "[100, 0, 99, 007]"], ["[1, 2, 3]", "[1,2, 3, 4]", "[1, 2, 3, 4444]", "[1, 2, 3, 4] ", "1, 2, 3, 4", "[a, 2, 3, 4]"]),
    GD.BOX_LIST_PATTERN: (["[1, 2, 3, 4]", "[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]"], ["[1, 2, 3, 4],", "[1, 2, 3, 4] [5, 6, 7, 8]", "[1, 2, 3, 4],[5, 6, 7, 8]", ""]),
    r"(cat|dog|bird)s?": (["cat", "dogs", "birds"], ["cats?", "catdog", "ca", "birdss", ""]),
    r"a(b|c(d|e)*f)+g": (["abg", "acfg", "acdedfbg"], ["ag", "acg", "abcg", "acdf"]),
    r"x{2,4}y{3}z{1,}": (["xxyyyz", "xxxxyyyzzzz"], ["xyyyz", "xxxxxyyyz", "xxyyz", "xxyyy"]),
    r"[^0-9\]]{1,5}\.": (["a.", "[abc,.", "....."], ["1.", "].", "abcdef.", "abc", "."]),
    r"(?:yes|no)( \w+){0,2}": (["yes", "no way", "yes it_is 42"], ["yes ", "no a b c", "maybe", "yes  it"]),
    r"\s?[A-Z][a-z]*": (["Airport", " Hangar", "A"], ["airport", "  Hangar", "AirPort", ""]),
    r"a.c\\": (["abc\\", "a c\\"], ["abc", "a\nc\\", "ac\\"]),
    r"(ab|a)(c|bc)d?": (["abc", "ac", "abbcd", "abcd"], ["ab", "abb", "acdd", "bc"]),
    r"[a-c\-x]+\d*": (["abc-x", "x12", "-"], ["d", "12", "ab_c"]),
}


@pytest.mark.parametrize("pattern", list(PATTERNS), ids=[f"p{i}" for i in range(len(PATTERNS))])
def test_from_regex_agrees_with_re(pattern):
    g = GD.TokenGuide.from_regex(pattern, BYTES, EOS)
    rx = re.compile(pattern.encode())
    good, bad = PATTERNS[pattern]
    for s in good:
        assert rx.fullmatch(s.encode()) and g.accepts(ids(s)), s
    for s in bad:
        assert not rx.fullmatch(s.encode()) and not g.accepts(ids(s)), s
    # every string spelled by a seeded random walk to END full-matches
    rng = random.Random(len(pattern))
    done = 0
    for _ in range(60):
        s, out = g.start, []
        while s != g.end and len(out) < 300:
            allowed = g.allowed(s)
            assert allowed, s
            t = EOS if (EOS in allowed and rng.random() < 0.3) else rng.choice(allowed)
            if t != EOS:
                out.append(t)
            s = g.step(s, t)
        if s == g.end:
            done += 1
            assert rx.fullmatch(spell(out)), (pattern, spell(out))
    assert done >= 20
    # END allows only EOS and loops; every state reaches END; nothing but an accepting state allows EOS
    assert g.allowed(g.end) == [EOS] and g.step(g.end, EOS) == g.end and g.end == g.n_states - 1
    reach = {g.end}
    for _ in range(g.n_states):
        reach |= {s for s in range(g.n_states) if any(q in reach for q in set(g.next[s].tolist()) - {GD.NONE})}
    assert reach == set(range(g.n_states))
    assert g.next.dtype == np.uint16 and g.next.shape == (g.n_states, 259) and g.table_bytes == g.n_states * 259 * 2
    for t in (0, 1):                                                  # <unk> / BOS are never allowed
        assert (g.next[:, t] == GD.NONE).all()


def test_the_box_constants_yield_only_what_the_two_parsers_accept():
    from teochat_amd.detection import boxes_from_response
    rng = random.Random(5)
    for pattern in (GD.BOX_PATTERN, GD.BOX_LIST_PATTERN):
        g = GD.TokenGuide.from_regex(pattern, BYTES, EOS)
        for _ in range(40):
            s, out = g.start, []
            while s != g.end:
                allowed = g.allowed(s)
                t = EOS if EOS in allowed and (len(out) > 60 or rng.random() < 0.5) else rng.choice([a for a in allowed if a != EOS] or [EOS])
                if t != EOS:
                    out.append(t)
                s = g.step(s, t)
            text = spell(out).decode()
            boxes = I.extract_bboxes(text)                           # r"\[(\d+), (\d+), (\d+), (\d+)\]"
            assert boxes and all(len(b) == 4 and all(0 <= v <= 999 for v in b) for b in boxes), text
            assert len(boxes_from_response(text, 256, 256)) == len(boxes) == text.count("[")        # r"\[(.*?)\]", split on ","


def test_unsupported_syntax_and_empty_languages_raise():
    for bad in (r"^a", r"a$", r"(?=a)b", r"a{3,2}", r"(a", r"a)", r"[a", r"*a", r"\1", r"a{,3}x{", r"a**", r"a*+", r"a{2}{3}", r"a+??"):
        with pytest.raises(ValueError):
            GD.TokenGuide.from_regex(bad, BYTES, EOS)
    with pytest.raises(ValueError):
        GD.TokenGuide.from_regex(r"abc", [None, None, None, b"a", b"b"], EOS)         # this vocabulary cannot spell it
    assert GD.TokenGuide.from_regex(r"a*?b+?", BYTES, EOS).accepts(ids("aabb"))          # lazy forms: the same strings in full


# --------------------------------------------------------------------------------------------------------------------- the token lift
def test_token_lift_equals_the_byte_by_byte_walk():
    pieces = [None, None, None] + [bytes([b]) for b in b"0123456789[], "] + [b"12", b", ", b"],", b"]", b"[1", b"345", b"], [", None, b"", b"x["]
    V = len(pieces)
    single = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, BYTES, EOS)                # the byte automaton
    g = GD.TokenGuide.from_regex(GD.BOX_LIST_PATTERN, pieces, EOS)
    assert g.vocab == V and g.n_states == single.n_states                             # every byte is a piece too: the same states survive
    # pair the states of the two automata by walking both from the start over single-byte pieces
    byte_tok = {p[0]: t for t, p in enumerate(pieces) if p is not None and len(p) == 1}
    pair, todo = {g.start: single.start}, [g.start]
    while todo:
        s = todo.pop()
        for b, t in byte_tok.items():
            q = g.step(s, t)
            if q is not None and q not in pair:
                pair[q] = single.step(pair[s], 3 + b)
                todo.append(q)
    inv = {v: k for k, v in pair.items()}
    assert len(pair) == g.n_states - 1 and len(inv) == len(pair)
    checked = 0
    for s, bs in pair.items():
        for t, p in enumerate(pieces):
            if t == EOS:
                continue
            want = single.walk([3 + b for b in p], bs) if p else None                 # byte by byte; None and b"" are never allowed
            got = g.step(s, t)
            assert got == (inv[want] if want is not None else None), (s, t, p)
            checked += got is not None
    assert checked > 40
    multi = [t for t, p in enumerate(pieces) if p and len(p) > 1]
    assert any(g.step(s, t) is not None for s in pair for t in multi)
    toks = [pieces.index(b"[1"), pieces.index(b", "), pieces.index(b"12"), pieces.index(b", "), pieces.index(b"345"), pieces.index(b", "),
            pieces.index(b"6"), pieces.index(b"], ["), pieces.index(b"7"), pieces.index(b", "), pieces.index(b"8"), pieces.index(b", "),
            pieces.index(b"9"), pieces.index(b", "), pieces.index(b"0"), pieces.index(b"]")]
    assert g.accepts(toks) and spell(toks, pieces) == b"[1, 12, 345, 6], [7, 8, 9, 0]"
    assert not g.accepts(toks[:-1]) and g.walk([pieces.index(b"x[")]) is None


def test_pieces_of_byte_and_sentencepiece_tokenizers():
    assert BYTES[:3] == [None, None, None] and BYTES[3 + 65] == b"A" and len(BYTES) == 259
    assert len(GD.pieces_of(ByteTokenizer(), 300)) == 300 and GD.pieces_of(ByteTokenizer(), 300)[259:] == [None] * 41
    with pytest.raises(ValueError):
        GD.pieces_of(ByteTokenizer(), 100)

    class SP:
        all_special_ids = [0, 1, 2]
        toks = ["<unk>", "<s>", "</s>", "<0x0A>", "<0xFF>", "▁the", "▁", "[", "12", "▁▁", "<image>", "é"]

        def __len__(self):
            return len(self.toks)

        def convert_ids_to_tokens(self, ids):
            return [self.toks[i] for i in ids]
    assert GD.pieces_of(SP()) == [None, None, None, b"\n", b"\xff", b" the", b" ", b"[", b"12", b"  ", None, "é".encode()]
    g = GD.named_guide("boxes", ByteTokenizer(), 300)
    assert g.vocab == 300 and g.accepts(ids("[1, 2, 3, 4], [5, 6, 7, 8]"))
    with pytest.raises(ValueError):
        GD.named_guide("json", ByteTokenizer())


# ------------------------------------------------------------------------------------------------ trie, GuideSet, constructor checks
def test_from_sequences_is_a_trie():
    seqs = [[10, 11, 12], [10, 11], [10, 20, 21], [30]]
    g = GD.TokenGuide.from_sequences(seqs, EOS, vocab=40)
    assert g.n_states == 8 and g.vocab == 40                           # root, 10, 10-11, 10-11-12, 10-20, 10-20-21, 30, END
    for s in seqs:
        assert g.accepts(s)
    for s in ([10], [10, 20], [10, 11, 12, 12], [11], []):
        assert not g.accepts(s)
    assert g.allowed(g.start) == [10, 30] and g.allowed(g.walk([10, 11])) == [EOS, 12]
    assert GD.TokenGuide.from_sequences(seqs, EOS).vocab == 31
    with pytest.raises(ValueError):
        GD.TokenGuide.from_sequences([[10, EOS]], EOS, vocab=40)
    with pytest.raises(ValueError):
        GD.TokenGuide.from_sequences([[]], EOS, vocab=40)


def test_guide_set_offsets_and_none_as_the_universal_automaton():
    a = GD.TokenGuide.from_sequences([[10, 11], [12]], EOS, vocab=40)
    b = GD.TokenGuide.from_regex(r"ab?", [None] * 3 + [b"a", b"b"] + [None] * 35, EOS)
    gs = GD.GuideSet([a, None, b, a, None], eos=EOS)
    assert gs.n_states == a.n_states + 1 + b.n_states and gs.next.shape == (gs.n_states, 40)
    assert gs.offsets == [0, a.n_states, a.n_states + 1, 0, a.n_states] and gs.starts == [0, a.n_states, a.n_states + 1, 0, a.n_states]
    for m, off in ((a, 0), (b, a.n_states + 1)):
        blk = gs.next[off:off + m.n_states]
        assert np.array_equal(blk == GD.NONE, m.next == GD.NONE)
        assert np.array_equal(blk[m.next != GD.NONE], m.next[m.next != GD.NONE] + off)
    uni = gs.next[a.n_states]
    assert (uni == a.n_states).all()                                   # everything allowed, EOS included, and it loops on itself
    only_none = GD.GuideSet([None, None], vocab=12)
    assert only_none.n_states == 1 and only_none.starts == [0, 0] and (only_none.next == 0).all()
    with pytest.raises(ValueError):
        GD.GuideSet([None])
    with pytest.raises(ValueError):
        GD.GuideSet([a, GD.TokenGuide.from_sequences([[1]], EOS, vocab=41)])
    u = GD.TokenGuide.universal(12, EOS)
    assert u.n_states == 1 and u.allowed(0) == list(range(12)) and u.table_bytes == 24


def test_constructor_prunes_and_raises():
    # state 2 loops on itself and never accepts: pruned, together with the transition into it; state 3 is unreachable
    g = GD.TokenGuide([{5: 1, 6: 2}, {7: 1}, {8: 2}, {9: 1}], [1], 0, 12, EOS)
    assert g.n_states == 3 and g.allowed(0) == [5] and g.allowed(1) == [EOS, 7] and g.end == 2
    # a reachable state that allows no token and is not accepting
    with pytest.raises(ValueError, match="allows no token"):
        GD.TokenGuide([{5: 1, 6: 2}, {}, {}], [1], 0, 12, EOS)
    # nothing accepting can be reached
    with pytest.raises(ValueError):
        GD.TokenGuide([{5: 0}], [], 0, 12, EOS)
    # EOS as an ordinary transition, a token outside the vocabulary, a successor that does not exist
    for trans in ([{EOS: 0}], [{12: 0}], [{5: 3}]):
        with pytest.raises(ValueError):
            GD.TokenGuide(trans, [0], 0, 12, EOS)
    # S > 65534 (END included)
    chain = [{5: i + 1} for i in range(GD.MAX_STATES - 1)] + [{}]
    with pytest.raises(ValueError, match="exceed"):
        GD.TokenGuide(chain, [len(chain) - 1], 0, 8, EOS)
    ok = GD.TokenGuide(chain[:200] + [{}], [200], 0, 8, EOS)
    assert ok.n_states == 202 and ok.accepts([5] * 200)
    with pytest.raises(ValueError):
        GD.GuideSet([ok] + [GD.TokenGuide(chain[:200] + [{}], [200], 0, 8, EOS) for _ in range(330)])


# ------------------------------------------------------------------------------------------------------------ the fourth header's table
GUIDE_HEADER = os.path.join(ROOT, "include", "teo_hip_guide.h")
GUIDE_CONTAINMENT = "tests/test_guide_gpu.py"
GUIDE_TABLE = {
    "teo_guide_sizeof": reason("host only: returns a number, takes no device pointer"),
    "teo_guide_mask": arena(GUIDE_CONTAINMENT),
    "teo_guide_advance": arena(GUIDE_CONTAINMENT),
    "teo_llama_decode_step_guided": arena(GUIDE_CONTAINMENT),
    "teo_llama_decode_graph_create_guided": arena(GUIDE_CONTAINMENT),
    "teo_llama_decode_stream_step_guided": arena(GUIDE_CONTAINMENT),
    "teo_llama_decode_stream_graph_create_guided": arena(GUIDE_CONTAINMENT),
}


def test_the_fourth_header_has_a_table_and_a_binding_of_its_own():
    header = open(GUIDE_HEADER).read()
    assert problems(header, table=GUIDE_TABLE) == []
    names = declared_functions(header)
    assert sorted(names) == sorted(L._SIGS_GUIDE) == sorted(L.EXPORTS_GUIDE) == sorted(GUIDE_TABLE)
    assert not set(names) & (set(L._SIGS) | set(L._SIGS_PREFIX) | set(L._SIGS_SCORE)), "a name of the fourth header is in another table"
    assert '#include "teo_hip.h"' in header
    for name in ("include/teo_hip.h", "include/teo_hip_prefix.h", "include/teo_hip_score.h", "teochat_amd/csrc/common.h", "teochat_amd/csrc/ops.h"):
        assert "teo_hip_guide.h" not in open(os.path.join(ROOT, name)).read(), name           # nothing existing includes it
    lib = L.load()
    for name in names:
        assert hasattr(lib, name), name
    assert lib.teo_version() == 4 == L.ABI_VERSION
    assert lib.teo_guide_sizeof() == 32
    fake = header.replace("int teo_guide_mask(", "int teo_brand_new_kernel(const void* d_x, void* d_y, int n);\nint teo_guide_mask(")
    assert problems(fake, table=GUIDE_TABLE) == ["teo_brand_new_kernel: declared in the header, no row in the table"]
    short = {k: v for k, v in GUIDE_TABLE.items() if k != "teo_guide_advance"}
    assert problems(header, table=short) == ["teo_guide_advance: declared in the header, no row in the table"]


# --------------------------------------------------------------------------------------------------------------------------- wiring
class Stub:
    """generate / generate_stream as the model has them: record the keywords, answer with EOS"""
    device, dtype = "cpu", torch.float32

    def __init__(self):
        self.calls = []

    def generate(self, input_ids=None, images=None, **kw):
        self.calls.append(("generate", kw))
        return torch.cat([input_ids, torch.tensor([[EOS]])], dim=1)

    def generate_stream(self, ids_list, images_list, **kw):
        guides = kw.get("guides")
        self.calls.append(("generate_stream", dict(kw, guides=[guides[i] for i in range(len(guides))] if guides is not None else None)))
        return [torch.cat([ids_list[i], torch.tensor([EOS])]) for i in range(len(ids_list))]


class Processor:
    def preprocess(self, path, return_tensors="pt"):
        return {"pixel_values": [torch.zeros(3, 2, 2)]}


def _data(n):
    return [{"conversations": [{"value": f"<video>\nQ{i}?"}, {"value": f"[1, 2, 3, {i}]"}], "video": ["img"], "timestamp": [], "task": "t"} for i in range(n)]


def test_run_inference_passes_the_guide_through():
    tok, model, proc = ByteTokenizer(), Stub(), Processor()
    g = GD.TokenGuide.from_regex(GD.BOX_PATTERN, BYTES, EOS)
    I.run_inference_single(model, proc, tok, "<video>\nQ?", ["img"], guide=g)
    assert model.calls[-1][1]["guide"] is g
    I.run_inference_single(model, proc, tok, "<video>\nQ?", ["img"])
    assert "guide" not in model.calls[-1][1]                            # not passed on unless asked for
    data = _data(3)
    # one guide for every example, batch size 1
    model.calls.clear()
    I.run_inference(data, model, tok, proc, "interleave", True, "v1", 0.2, 8, guide=g)
    assert [c[1]["guide"] for c in model.calls] == [g, g, g]
    # a callable per example, continuous: generate_stream(guides=...)
    model.calls.clear()
    other = GD.TokenGuide.from_sequences([[70]], EOS, vocab=259)
    I.run_inference(data, model, tok, proc, "interleave", True, "v1", 0.2, 8, batch_size=2, continuous=True,
                    guide=lambda e: other if e["conversations"][1]["value"].endswith("1]") else (None if e["conversations"][1]["value"].endswith("2]") else g))
    assert model.calls[-1][0] == "generate_stream" and model.calls[-1][1]["guides"] == [g, other, None]
    model.calls.clear()
    I.run_inference(data, model, tok, proc, "interleave", True, "v1", 0.2, 8, batch_size=2, continuous=True)
    assert model.calls[-1][1]["guides"] is None
    with pytest.raises(ValueError):
        I.run_inference(data, model, tok, proc, "interleave", True, "v1", 0.2, 8, batch_size=2, guide=g)
    with pytest.raises(ValueError):
        I.run_inference_batch(model, proc, tok, ["<video>\nQ?"], [["img"]], guides=[g])


def test_the_eval_switch_builds_the_box_guide(tmp_path):
    from teochat_amd import eval as E
    assert vars(E.cli_parser().parse_args(["--dataset_name", "xbd_loc", "--model_path", "m", "--guide", "boxes"]))["guide"] == "boxes"
    assert "guide" not in vars(E.cli_parser().parse_args(["--dataset_name", "xbd_loc", "--model_path", "m"]))
    with pytest.raises(SystemExit):
        E.cli_parser().parse_args(["--dataset_name", "xbd_loc", "--model_path", "m", "--guide", "json"])
    tok, model, proc = ByteTokenizer(), Stub(), Processor()
    data = [dict(e, task="qa") for e in _data(2)]
    E.eval("cdvqa", "stub-model", None, out_dir=str(tmp_path), dataset=data, model_bundle=(tok, model, proc), guide="boxes", max_new_tokens=8)
    guides = [c[1]["guide"] for c in model.calls]
    assert len(guides) == 2 and guides[0] is guides[1] and guides[0].accepts(ids("[1, 2, 3, 4], [5, 6, 7, 8]")) and not guides[0].accepts(ids("[1, 2]"))
