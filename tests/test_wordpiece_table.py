"""The fold table of the BERT tokenizer (csrc/kernels/wordpiece_table.h, read
through tests/wordpiece_cases.py): it is what tools/make_wordpiece_tables.py
writes, no fold is longer than 3 or longer than its source has bytes, and every
class rule of csrc/kernels/wordpiece_core.h holds for every code point against
``unicodedata``.  The checks against ``unicodedata`` need this Python's Unicode
version to be the one the table records; otherwise they are skipped with the
reason, and the structural checks still run."""

import importlib.util
import os
import unicodedata as ud

import pytest

from tests import wordpiece_cases as wc

CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
       (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
ASCII_PUNCT = set(range(33, 48)) | set(range(58, 65)) | set(range(91, 97)) | set(range(123, 127))


def _same_unicode():
    if wc.table().unicode_version != ud.unidata_version:
        pytest.skip("the table records Unicode %s, this Python has %s" % (wc.table().unicode_version,
                                                                          ud.unidata_version))


def _generator():
    spec = importlib.util.spec_from_file_location("make_wordpiece_tables",
                                                  os.path.join(wc.REPO, "tools", "make_wordpiece_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_committed_table_is_a_fresh_run_of_the_generator():
    _same_unicode()
    assert open(wc.TABLE_H).read() == _generator().render()


def test_no_fold_is_longer_than_3_or_than_its_source():
    tab = wc.table()
    assert len(tab.stage1) == 0x110000 >> 7 and len(tab.stage2) % 128 == 0
    longest = 0
    for cp in range(0x110000):
        f = tab.fold(cp)
        if f == wc.SPACE:
            continue
        nbytes = 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4
        assert len(f) <= 3 and len(f) <= nbytes, hex(cp)
        assert all(0 < x <= 0x10FFFF for x, _ in f), hex(cp)
        longest = max(longest, len(f))
    assert longest == 3


def _is_punct(cp):
    return cp in ASCII_PUNCT or ud.category(chr(cp)).startswith("P")


def test_every_class_rule_holds_for_every_code_point():
    _same_unicode()
    tab = wc.table()
    counts = {"drop": 0, "space": 0, "cjk": 0, "punct": 0, "fold": 0}
    for cp in range(0x110000):
        if 0xD800 <= cp <= 0xDFFF:
            assert tab.fold(cp) == [], hex(cp)  # never decoded from valid UTF-8
            continue
        c = chr(cp)
        cat = ud.category(c)
        f = tab.fold(cp)
        if c in "\t\n\r" or cat == "Zs" or cp in (0x2028, 0x2029):
            assert f == wc.SPACE, hex(cp)
            counts["space"] += 1
            continue
        if cp in (0, 0xFFFD) or cat in ("Cc", "Cf", "Cn", "Co"):
            assert f == [], hex(cp)
            counts["drop"] += 1
            continue
        want = []
        for x in ud.normalize("NFD", c):
            if ud.category(x) == "Mn":
                continue
            low = x.lower()
            want.append(ord(low) if len(low) == 1 else ord(x))
        assert [x for x, _ in f] == want, hex(cp)
        cjk = any(a <= cp <= b for a, b in CJK)
        is_space, is_cjk, punct = tab.classes(cp)
        assert not is_space and is_cjk == cjk and punct == [_is_punct(x) for x in want], hex(cp)
        # a word of its own: punctuation or an ideograph, and nothing else
        assert [own for _, own in f] == [p or cjk for p in punct], hex(cp)
        if cjk:
            assert len(want) == 1 and any(a <= want[0] <= b for a, b in CJK), hex(cp)
        counts["cjk" if cjk else "punct" if any(punct) else "fold"] += 1
    assert all(counts.values()), counts
    # the rule's corner stones
    assert tab.fold(0x3A3) == [(0x3C3, False)] and tab.fold(0x3C2) == [(0x3C2, False)]  # no final-sigma rule
    assert tab.fold(0x130) == [(ord("i"), False)] and tab.fold(0xF900) == [(0x8C48, True)]
    assert tab.fold(0xAC00) == [(0x1100, False), (0x1161, False)] and len(tab.fold(0xAC01)) == 3
    assert tab.fold(0x37E) == [(ord(";"), True)] and tab.fold(0x2260) == [(ord("="), True)]


def test_the_host_library_folds_as_the_table_says():
    from triton_client_amd.ops import host_codec

    codec = host_codec.load()
    tab = wc.table()
    for cp in list(range(0x3100)) + list(range(0xAC00, 0xAC40)) + list(range(0xF900, 0xFB00)) + [0x1F600, 0x20000,
                                                                                                 0x2F800, 0x10FFFF]:
        f = tab.fold(cp)
        want = [1 << 31] if f == wc.SPACE else [x | (1 << 30 if own else 0) for x, own in f]
        assert codec.wordpiece_fold(cp) == want, hex(cp)
    with pytest.raises(ValueError):
        codec.wordpiece_fold(0x110000)
