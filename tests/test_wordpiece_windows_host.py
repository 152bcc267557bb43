"""K28w's host twins (csrc/host/wordpiece.cc tcamd_host_wordpiece_windows and
its phase-by-phase emulation) against the Python twin of
tests/wordpiece_window_cases.py: exact equality on every output word, the
slice and start-mask properties, a single window against
``HostCodec.wordpiece_tokenize``, and the client's ``doc_windows``."""

import numpy as np
import pytest

from tests import wordpiece_cases as wc
from tests import wordpiece_window_cases as ww


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


def _three_ways(codec, vocab, twin_vocab, qs, cs, mq, ds, mw, S, out_rows, what):
    want, pieces_of = ww.window_rows(qs, cs, twin_vocab, mq, ds, mw, S, out_rows)
    walk = codec.wordpiece_windows(qs, cs, vocab, mq, ds, mw, S, out_rows)
    phases = codec.wordpiece_windows(qs, cs, vocab, mq, ds, mw, S, out_rows, emulate=True)
    ww.assert_same(walk, want, what + " (walk)")
    ww.assert_same(phases, want, what + " (phases)")
    ww.assert_properties(walk, pieces_of, S)
    return want


@pytest.mark.parametrize("case", ww.small_cases(), ids=lambda c: c[0])
def test_small_cases_three_ways(codec, vocab, twin_vocab, case):
    name, qs, cs, mq, ds, mw, out_rows = case
    want = _three_ways(codec, vocab, twin_vocab, qs, cs, mq, ds, mw, 12, out_rows, name)
    dinfo = want[6]
    if name.startswith("P "):
        P, stride = int(name.split()[1]), min(int(name.split()[3]), 7)
        assert dinfo[0, 2] == P and dinfo[0, 3] == 0
        assert dinfo[0, 1] == (1 if P <= 7 else -(-(P - 7) // stride) + 1)
    if name == "one below max_windows":
        assert [int(x) for x in dinfo[0]] == [0, 6, 20, ww.ST_WINDOWS] and [int(x) for x in dinfo[1]] == [0, 1, 5, 0]
    if name == "invalid between":
        assert dinfo[1, 3] == wc.status_word(wc.ST_INVALID, 1, 2) and dinfo[0, 3] == 0 and dinfo[2, 3] == 0
        assert dinfo[2, 0] == dinfo[0, 1]  # the refused document owns no row
    if name == "cap 0":
        assert [int(x) for x in dinfo[0]] == [0, ww.NEVER, 3, ww.ST_WINDOWS] and [int(x) for x in dinfo[1]] == [0, 1, 0, 0]
    if name == "small capacity":
        assert [int(x) for x in dinfo[:, 3]] == [0, ww.ST_WINDOWS, ww.ST_WINDOWS] and want[7] == 2


@pytest.mark.parametrize("total", [128, 129])
def test_row_capacity(codec, vocab, twin_vocab, total):
    qs, cs, mq, ds, mw, out_rows = ww.capacity_case(total)
    want = _three_ways(codec, vocab, twin_vocab, qs, cs, mq, ds, mw, 12, out_rows, "capacity %d" % total)
    dinfo = want[6]
    assert (dinfo[:127, 3] == 0).all() and (dinfo[:127, 0] == np.arange(127)).all()
    assert dinfo[127, 3] == (0 if total == 128 else ww.ST_WINDOWS) and want[7] == (128 if total == 128 else 127)


@pytest.mark.parametrize("nbytes", [1100, 2100, 4096])
def test_long_contexts_at_the_served_shape(codec, vocab, twin_vocab, nbytes):
    qs = [b"What is tokenization?", "Σσ привет".encode()]
    cs = [ww.long_context(nbytes, nbytes), ww.long_context(nbytes // 2, 7)]
    want = _three_ways(codec, vocab, twin_vocab, qs, cs, [64, 3], [128, 50], 128, 384, 128, "long %d" % nbytes)
    assert want[6][0, 1] > 1 or nbytes < 4000


def test_random_documents(codec, vocab, twin_vocab):
    for seed in range(6):
        qs, cs, mq = wc.random_rows(100 + seed, 9, max_items=120)
        rng = np.random.default_rng(seed)
        ds = rng.integers(1, 30, size=9)
        mw = rng.choice([128, 128, 3, 1], size=9)
        _three_ways(codec, vocab, twin_vocab, qs, cs, np.minimum(mq, 29), ds, mw, 32, 64, "random %d" % seed)


def test_a_single_window_is_the_row_of_wordpiece_tokenize(codec, vocab):
    qs = [b"What is the answer?", "Σσ Привет".encode(), b"", b"a a a a"]
    cs = ["The quick brown fox jumps over the lazy dog. café".encode(), "中国 tokenization 한글".encode(), b"walked",
          b"b " * 377]
    ids, mask, tt, offsets, overflow, status = codec.wordpiece_tokenize(qs, cs, vocab, 64, 384)
    assert not status.any() and not overflow.any()
    got = codec.wordpiece_windows(qs, cs, vocab, 64, 128, 128, 384, 128)
    assert got[7] == 4 and (got[6][:, 1] == 1).all()
    for g, w in zip((got[0], got[1], got[2], got[4]), (ids, mask, tt, offsets)):
        np.testing.assert_array_equal(g[:4], w)
    np.testing.assert_array_equal(got[3][:4], tt)  # one window: every context piece may start


def test_what_the_entry_refuses(codec, vocab):
    with pytest.raises(ValueError):
        codec.wordpiece_windows([b"a"], [b"b"], vocab, out_rows=129)
    with pytest.raises(ValueError):
        codec.wordpiece_windows([b"a"], [b"b"], vocab, out_rows=0)
    with pytest.raises(ValueError):
        codec.wordpiece_windows([b"a"], [b"b"], vocab, S=3)
    with pytest.raises(ValueError):
        codec.wordpiece_windows([b"a"], [b"b"], vocab, emulate=True, workspace_bytes=64)


def test_doc_windows_of_the_client_is_the_rule():
    from triton_client_amd.utils.qa import doc_windows

    for P in (0, 1, 7, 8, 10, 11, 50, 400, 1000):
        for qn, stride, S in ((2, 1, 12), (2, 3, 12), (2, 7, 12), (2, 9, 12), (5, 128, 384), (64, 128, 384)):
            starts, lens, best = ww.windows_of(P, S - 3 - qn, stride)
            g_starts, g_lens, g_best = doc_windows(P, qn, stride, S)
            assert list(g_starts) == starts and list(g_lens) == lens and list(g_best) == best, (P, qn, stride, S)
