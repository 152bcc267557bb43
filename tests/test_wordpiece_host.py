"""The host twin of K28 wordpiece (csrc/host/wordpiece.cc, through
``HostCodec.wordpiece_tokenize``) against the Python twin of
tests/wordpiece_cases.py: ids, mask, type ids, offsets, overflow and status,
exactly, on the fixed cases and on seeded random rows, both by the front-to-back
walk and by the emulation of the kernel's phases in the kernel's workspace
layout; vocabulary loading; and the Python twin against the ``tokenizers``
library (where it is installed) and against its recorded results (everywhere)."""

import json
import random

import numpy as np
import pytest

from tests import wordpiece_cases as wc


@pytest.fixture(scope="module")
def codec():
    from triton_client_amd.ops import host_codec

    return host_codec.load()


@pytest.fixture(scope="module")
def vocab():
    from triton_client_amd.utils import wordpiece

    return wordpiece.Vocab.load(wc.VOCAB_SMALL)


@pytest.fixture(scope="module")
def twin_vocab():
    return wc.TwinVocab()


@pytest.fixture(scope="module")
def fixed(twin_vocab):
    cases = wc.fixed_cases()
    cols = [c[1] for c in cases], [c[2] for c in cases], np.asarray([c[3] for c in cases], dtype=np.int32)
    return cases, cols, wc.tokenize_rows(*cols[:2], twin_vocab, cols[2])


@pytest.mark.parametrize("emulate", [False, True], ids=["walk", "phases"])
def test_host_twin_equals_the_python_twin_on_the_fixed_cases(codec, vocab, fixed, emulate):
    cases, (qs, cs, mq), want = fixed
    got = codec.wordpiece_tokenize(qs, cs, vocab, mq, emulate=emulate)
    for r, case in enumerate(cases):
        wc.assert_same([g[r:r + 1] for g in got], [w[r:r + 1] for w in want], case[0])


def test_the_fixed_cases_reach_what_they_are_named_for(fixed, twin_vocab):
    cases, _, (ids, mask, tt, offsets, overflow, status) = fixed
    by = {c[0]: r for r, c in enumerate(cases)}
    S, unk = wc.SEQ, twin_vocab.unk

    def pieces(name):
        r = by[name]
        return [int(x) for x in ids[r][mask[r] == 1]]

    assert pieces("empty both") == [twin_vocab.cls, twin_vocab.sep, twin_vocab.sep]
    assert pieces("all space") == pieces("dropped only") == pieces("empty both")
    assert pieces("word of 100")[1] == twin_vocab.pieces.index("x" * 100) and unk not in pieces("word of 100")
    assert pieces("word of 101")[1] == unk and pieces("word of 101").count(unk) == 4
    assert unk in pieces("unknown tail") and twin_vocab.pieces.index("αβγ") in pieces("unknown tail")
    assert pieces("question exactly max") == pieces("question one more")
    r = by["context fills the row"]
    assert mask[r].all() and overflow[r] == 0 and tt[r].sum() == S - 5 and ids[r, S - 1] == twin_vocab.sep
    r = by["context overflows by one"]
    assert mask[r].all() and overflow[r] == 1
    assert tt[by["max_query_length 1"]].argmax() == 3
    r = by["max_query_length S-3"]
    assert mask[r].all() and tt[r].sum() == 0 and overflow[r] == 2 and ids[r, S - 1] == ids[r, S - 2] == twin_vocab.sep
    # token_type_ids is 1 on the context pieces alone, offsets are non-zero there alone
    assert ((offsets[..., 1] > 0) == (tt == 1)).all()
    assert status[by["text of 65536"]] == 0 and status[by["text of 65537"]] == wc.status_word(wc.ST_TOO_LONG, 1)
    assert status[by["question of 65537"]] == wc.status_word(wc.ST_TOO_LONG, 0)
    assert status[by["max_query_length 0"]] == status[by["max_query_length S-2"]] == wc.ST_PARAM
    bad = [r for r, c in enumerate(cases) if c[0].startswith("invalid")]
    assert len(bad) == 13 * 4 and all(status[r] & 0xFF == wc.ST_INVALID and not mask[r].any() for r in bad)
    assert status[by["invalid surrogate first"]] == wc.status_word(wc.ST_INVALID, 1, 0)
    assert status[by["invalid surrogate mid"]] == wc.status_word(wc.ST_INVALID, 1, len("head é中".encode()))
    assert status[by["invalid truncated 3 last"]] == wc.status_word(wc.ST_INVALID, 1, len("head é".encode()))
    assert status[by["invalid surrogate question"]] == wc.status_word(wc.ST_INVALID, 0, 2)
    # a fold of 2 and 3 code points keeps the offsets of its one source
    e, jamo = twin_vocab.pieces.index("e"), [twin_vocab.pieces.index(p) for p in ("\u1112\u1161", "##\u11ab")]
    assert wc.tokenize_text("\u00e9".encode(), twin_vocab)[0] == [(e, 0, 2)]  # two bytes, one folded code point
    assert wc.tokenize_text("e\u0301".encode(), twin_vocab)[0] == [(e, 0, 1)]  # the mark folds to nothing
    assert wc.tokenize_text("\ud55c".encode(), twin_vocab)[0] == [(j, 0, 3) for j in jamo]  # one source, two pieces
    assert unk not in pieces("fold to 0 2 3")[:3]


@pytest.mark.parametrize("seed", range(6))
def test_host_twin_equals_the_python_twin_on_random_rows(codec, vocab, twin_vocab, seed):
    qs, cs, mq = wc.random_rows(seed, 500)
    want = wc.tokenize_rows(qs, cs, twin_vocab, mq)
    for first in range(0, 500, 125):  # the phases take 128 rows a call
        part = slice(first, first + 125)
        for emulate in (False, True):
            got = codec.wordpiece_tokenize(qs[part], cs[part], vocab, mq[part], emulate=emulate)
            wc.assert_same(got, [w[part] for w in want], "seed %d rows %d.. emulate=%s" % (seed, first, emulate))
    assert (want[5] != 0).any() and (want[0] == twin_vocab.unk).any()


def test_the_phases_cross_chunk_edges_as_the_walk_does(codec, vocab, twin_vocab):
    C = codec.wordpiece_geometry()["chunk"]
    texts = [("한" * (C // 3 + 5) + " 글").encode(), ("a " * (C // 2 - 3) + "tokenization walked").encode(),
             ("b " * (C // 2 - 20) + "x" * 100 + " " + "x" * 101 + " end").encode(),
             ("a" * (C - 1)).encode() + b"\xe2\x82", ("a " * ((C - 2) // 2) + "\U0001f600 tail").encode(),
             ("​" * 7 + "한글" * (C // 6 + 3)).encode(), (b"ab " * 21846)[:65536]]
    want = wc.tokenize_rows([b"q"] * len(texts), texts, twin_vocab, 64)
    wc.assert_same(codec.wordpiece_tokenize([b"q"] * len(texts), texts, vocab, 64, emulate=True), want, "context")
    want = wc.tokenize_rows(texts, [b"c"] * len(texts), twin_vocab, 381)
    wc.assert_same(codec.wordpiece_tokenize(texts, [b"c"] * len(texts), vocab, 381, emulate=True), want, "question")


def test_what_the_entry_refuses_and_what_a_short_workspace_does(codec, vocab):
    with pytest.raises(ValueError):
        codec.wordpiece_tokenize([b"a"] * 129, [b"b"] * 129, vocab, emulate=True)
    with pytest.raises(ValueError):
        codec.wordpiece_tokenize([b"a"], [b"b"], vocab, S=3)
    with pytest.raises(ValueError):
        codec.wordpiece_tokenize([b"a"], [b"b"], vocab, emulate=True, workspace_bytes=64)
    assert all(a.shape[0] == 0 for a in codec.wordpiece_tokenize([], [], vocab))
    # a workspace that holds the first row only: the second is refused in its status word, nothing is overrun
    need = codec.wordpiece_workspace(2, 8)
    assert need == codec.wordpiece_workspace(1, 8) and need > codec.wordpiece_workspace(2, 7)
    got = codec.wordpiece_tokenize([b"ab", b"ab"], [b"cd", b"cd"], vocab, emulate=True,
                                   workspace_bytes=codec.wordpiece_workspace(2, 6))
    assert got[5][0] == 0 and got[5][1] & 0xFF == wc.ST_RANGE and not got[1][1].any()
    broken = type("V", (), {"image": vocab.image.copy()})()
    broken.image[0] ^= 1
    assert (codec.wordpiece_tokenize([b"a"], [b"b"], broken)[5] & 0xFF == 5).all()
    assert (codec.wordpiece_tokenize([b"a"], [b"b"], broken, emulate=True)[5] & 0xFF == 5).all()


# ---- vocabulary loading ----------------------------------------------------------------------
def _write(tmp_path, lines, name="vocab.txt", end="\n"):
    p = tmp_path / name
    p.write_bytes(end.join(lines).encode("utf-8") + end.encode())
    return str(p)


def test_vocabulary_loading(codec, tmp_path, vocab):
    from triton_client_amd.utils import wordpiece

    assert (vocab.pad, vocab.unk, vocab.cls, vocab.sep) == (0, 1, 2, 3) and vocab.longest == 104
    assert vocab.duplicates == 0 and vocab.empty == 0
    assert vocab.unreachable == 7  # 한 ##글 (precomposed), Hello, é, ##É, ß, ##ß ... see the count below
    assert vocab.image.dtype == np.uint32 and vocab.image[0] == wordpiece.MAGIC and vocab.image[6] == vocab.image.size
    base = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "a", "##b"]
    for missing in range(4):
        lines = [p for k, p in enumerate(base) if k != missing]
        with pytest.raises(ValueError, match=r"lacks \%s" % base[missing].replace("]", r"\]")):
            wordpiece.Vocab.load(_write(tmp_path, lines))
    # a duplicate piece: the later id wins, as in a dict; an empty line keeps its id and never matches
    v = wordpiece.Vocab.load(_write(tmp_path, base + ["a", "", "c"], end="\r\n"))
    assert (v.duplicates, v.empty, len(v.pieces)) == (1, 1, 9)
    ids = codec.wordpiece_tokenize([b"a c"], [b"ab"], v)[0][0]
    assert list(ids[:7]) == [2, 6, 8, 3, 6, 5, 3]
    with pytest.raises(ValueError, match="not valid UTF-8"):
        p = tmp_path / "bad.txt"
        p.write_bytes(b"[PAD]\n\xff\n")
        wordpiece.Vocab.load(str(p))
    with pytest.raises(ValueError, match="1 to 2\\^20"):
        wordpiece.Vocab([])


def test_the_demonstration_vocabulary(codec):
    from triton_client_amd.utils import wordpiece

    assert wordpiece.default_vocab_path() == wordpiece.DEMO_VOCAB
    v = wordpiece.Vocab.load(wordpiece.DEMO_VOCAB)
    assert 1000 < len(v.pieces) < 30522 and v.image.nbytes < 1 << 20
    assert open(wordpiece.DEMO_VOCAB, "rb").read().__len__() < 64 * 1024
    for c in range(33, 127):
        assert chr(c) in v.pieces and "##" + chr(c) in v.pieces
    ids, mask, _, _, _, status = codec.wordpiece_tokenize([b"What does the kernel do?"],
                                                          [b"The kernel folds, matches and assembles rows."], v)
    assert not status.any() and v.unk not in ids[0] and 8 < mask[0].sum() < 40 and ids.max() < 30522


# ---- the library --------------------------------------------------------------------------------
def test_python_twin_equals_the_recorded_library_results(twin_vocab):
    doc = json.load(open(wc.GOLDEN))
    assert len(doc["cases"]) == 40
    for case in doc["cases"]:
        got, err = wc.tokenize_text(bytes.fromhex(case["text"]), twin_vocab)
        assert err is None
        assert [p[0] for p in got] == case["ids"] and [[p[1], p[2]] for p in got] == case["offsets"], case["text"]


def test_host_twin_equals_the_recorded_library_results(codec, vocab):
    cases = json.load(open(wc.GOLDEN))["cases"]
    for first in range(0, len(cases), 100):
        part = cases[first:first + 100]
        ids, mask, tt, offsets, overflow, status = codec.wordpiece_tokenize(
            [b""] * len(part), [bytes.fromhex(c["text"]) for c in part], vocab)
        assert not status.any() and not overflow.any()
        for r, c in enumerate(part):
            n = len(c["ids"])
            assert list(ids[r, 2:2 + n]) == c["ids"] and tt[r].sum() == n
            assert offsets[r, 2:2 + n].tolist() == c["offsets"]


def test_python_twin_equals_the_tokenizers_library_on_random_text(twin_vocab):
    pytest.importorskip("tokenizers")
    tok = wc.library_tokenizer()
    rng = random.Random(4242)
    seen_unk = False
    for n in range(2000):
        text = wc.random_text(rng)
        got, err = wc.tokenize_text(text.encode("utf-8"), twin_vocab)
        assert err is None
        assert [list(p) for p in got] == wc.library_pieces(tok, text), repr(text)  # no row is left out
        seen_unk = seen_unk or any(p[0] == twin_vocab.unk for p in got)
    assert seen_unk


def test_the_library_agrees_on_every_assigned_code_point_of_the_blocks(twin_vocab):
    pytest.importorskip("tokenizers")
    tok = wc.library_tokenizer()
    for lo, hi in ((0x0000, 0x024F), (0x0300, 0x03FF), (0x2000, 0x206F), (0x3000, 0x30FF), (0xF900, 0xFAFF),
                   (0xFF00, 0xFFEF), (0x1F600, 0x1F64F)):
        chars = [chr(cp) for cp in range(lo, hi + 1) if wc.assigned(cp)]
        text = "".join("a%sb " % c for c in chars)
        got, err = wc.tokenize_text(text.encode("utf-8"), twin_vocab)
        assert err is None and [list(p) for p in got] == wc.library_pieces(tok, text), hex(lo)


def test_the_stand_alone_cpp_test_passes():
    """csrc/cpp/tests/wordpiece_test.cc, as the project's build makes it (the
    ``asan`` preset builds the same source with the sanitizers)."""
    import os
    import subprocess

    exe = os.path.join(wc.REPO, "csrc", "cpp", "build", "bin", "wordpiece_test")
    assert os.path.exists(exe), "csrc/cpp is not built"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith(" 0 failures"), r.stdout[-2000:] + r.stderr[-2000:]
