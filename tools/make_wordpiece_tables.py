#!/usr/bin/env python3
"""Generate csrc/kernels/wordpiece_table.h, the fold table of the BERT
tokenizer (K28 wordpiece, its host twin and the Python twin all read it; the
rule is in csrc/kernels/wordpiece_core.h).

    python tools/make_wordpiece_tables.py            # rewrite the header
    python tools/make_wordpiece_tables.py --check    # exit 1 if it would change

The table is built from this Python's ``unicodedata``; the Unicode version goes
into the header comment, and tests/test_wordpiece_table.py compares the
committed file with a fresh run only where the versions agree.

Layout: ``stage1[cp >> 7]`` names a block, ``stage2[block * 128 + (cp & 127)]``
an entry (the header holds both stages as runs, ``(value, count)`` pairs, which
the compiler expands into ``kWpStages``), ``kWpEntries[entry]`` is one 32-bit
word:

    bits 0-20   n == 1: (folded - cp) mod 2^21;  n >= 2: index into kWpExt
    bits 21-22  n, the folded code points this one gives (0..3)
    bit 23      space (n == 0)
    bit 24      punct, of the folded code point (n == 1)
    bit 25      CJK ideograph: a word of its own (n == 1)
    bit 26      Hangul syllable: two jamo, or three when (cp - AC00) % 28 != 0, from arithmetic

``kWpExt`` holds the folds of two and three code points that are not Hangul:
one word per folded code point, the code point in bits 0-20 and its punct bit
in bit 24.  n == 0 without the space bit is a dropped code point.
"""
import argparse
import os
import sys
import unicodedata as ud

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "csrc", "kernels", "wordpiece_table.h")

N_SHIFT, SPACE, PUNCT, CJK, HANGUL = 21, 1 << 23, 1 << 24, 1 << 25, 1 << 26
MASK21 = (1 << 21) - 1
CJK_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
              (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
ASCII_PUNCT = set(range(33, 48)) | set(range(58, 65)) | set(range(91, 97)) | set(range(123, 127))


def is_cjk(cp):
    return any(a <= cp <= b for a, b in CJK_RANGES)


def is_punct(cp):
    return cp in ASCII_PUNCT or ud.category(chr(cp)).startswith("P")


def classify(cp):
    """('drop' | 'space' | 'fold', [folded code points]) by the rule, from unicodedata."""
    if 0xD800 <= cp <= 0xDFFF:
        return "drop", []  # never decoded from valid UTF-8; category Cs
    c = chr(cp)
    if c in "\t\n\r":
        return "space", []
    cat = ud.category(c)
    if cp == 0 or cp == 0xFFFD or cat in ("Cc", "Cf", "Cn", "Co"):
        return "drop", []
    if cat == "Zs" or cp in (0x2028, 0x2029):
        return "space", []
    out = []
    for x in ud.normalize("NFD", c):
        if ud.category(x) == "Mn":
            continue
        low = x.lower()
        out.append(ord(low) if len(low) == 1 else ord(x))  # the single-code-point mapping
    return "fold", out


def build():
    entries, entry_of, ext = [], {}, []
    stage2_blocks, block_of, stage1 = [], {}, []
    per_cp = []
    for cp in range(0x110000):
        kind, f = classify(cp)
        if len(f) > 3:
            raise SystemExit("U+%04X folds to %d code points" % (cp, len(f)))
        if len(f) > len(chr(cp).encode("utf-8", "surrogatepass")):
            raise SystemExit("U+%04X folds to more code points than it has bytes" % cp)
        if kind == "space":
            e = SPACE
        elif not f:
            e = 0
        elif 0xAC00 <= cp <= 0xD7A3:
            s = cp - 0xAC00
            jamo = [0x1100 + s // 588, 0x1161 + (s % 588) // 28] + ([0x11A7 + s % 28] if s % 28 else [])
            if f != jamo or any(is_punct(x) for x in f):
                raise SystemExit("U+%04X: Hangul arithmetic disagrees with unicodedata" % cp)
            e = HANGUL | (2 << N_SHIFT)  # one entry for all: the third jamo follows from arithmetic too
        elif len(f) == 1:
            e = ((f[0] - cp) & MASK21) | (1 << N_SHIFT) | (PUNCT if is_punct(f[0]) else 0) | (CJK if is_cjk(cp) else 0)
        else:
            if is_cjk(cp):
                raise SystemExit("U+%04X: a CJK ideograph with a fold of %d" % (cp, len(f)))
            words = tuple(x | (PUNCT if is_punct(x) else 0) for x in f)
            e = ("ext", words)
        per_cp.append(e)
    # the ext pool, then the entries
    ext_at = {}
    for e in per_cp:
        if isinstance(e, tuple) and e[1] not in ext_at:
            ext_at[e[1]] = len(ext)
            ext.extend(e[1])
    ids = []
    for e in per_cp:
        if isinstance(e, tuple):
            e = ext_at[e[1]] | (len(e[1]) << N_SHIFT)
        if e not in entry_of:
            entry_of[e] = len(entries)
            entries.append(e)
        ids.append(entry_of[e])
    for b in range(0x110000 >> 7):
        blk = tuple(ids[b * 128:(b + 1) * 128])
        if blk not in block_of:
            block_of[blk] = len(stage2_blocks)
            stage2_blocks.append(blk)
        stage1.append(block_of[blk])
    if len(entries) > 0xFFFF or len(stage2_blocks) > 0xFFFF:
        raise SystemExit("the table outgrew 16-bit indices")
    return stage1, [x for blk in stage2_blocks for x in blk], entries, ext


def _array(qual, ctype, name, vals, fmt, per_line):
    lines = ["%s %s %s[%d] = {" % (qual, ctype, name, len(vals))]
    for i in range(0, len(vals), per_line):
        lines.append("    " + ",".join(fmt % v for v in vals[i:i + per_line]) + ",")
    lines.append("};")
    return "\n".join(lines)


def _runs(vals):
    """``vals`` as (value, count) pairs, flat."""
    out = []
    for v in vals:
        if out and out[-2] == v and out[-1] < 0xFFFF:
            out[-1] += 1
        else:
            out += [v, 1]
    return out


def render():
    stage1, stage2, entries, ext = build()
    head = """// GENERATED by tools/make_wordpiece_tables.py -- do not edit.
// Unicode version: %s
//
// The fold table of the BERT tokenizer: per code point 0..10FFFF what it folds
// to and its class, by the rule in kernels/wordpiece_core.h.  K28
// (kernels/wordpiece.hip), the host twin (host/wordpiece.cc) and the Python
// twin (tests/wordpiece_cases.py) read these arrays and nothing else, so they
// agree on every code point whatever Unicode a machine's Python has.  The two
// stages are written as runs, (value, count) pairs, and expanded by the
// compiler into kWpStages; the layout is described in the generator and in
// wordpiece_core.h.
#pragma once

#include <stdint.h>

#ifndef TCAMD_WP_TABLE_ATTR
#define TCAMD_WP_TABLE_ATTR static
#endif

""" % ud.unidata_version
    r1, r2 = _runs(stage1), _runs(stage2)
    tail = """

constexpr int kWpStage1Len = %d, kWpStage2Len = %d;

struct WpStages {
  uint16_t stage1[kWpStage1Len];
  uint16_t stage2[kWpStage2Len];
};

constexpr WpStages wp_expand_stages() {
  WpStages s{};
  int at = 0;
  for (int i = 0; i < %d; i += 2)
    for (int k = 0; k < kWpStage1Runs[i + 1]; ++k) s.stage1[at++] = kWpStage1Runs[i];
  at = 0;
  for (int i = 0; i < %d; i += 2)
    for (int k = 0; k < kWpStage2Runs[i + 1]; ++k) s.stage2[at++] = kWpStage2Runs[i];
  return s;
}

TCAMD_WP_TABLE_ATTR constexpr WpStages kWpStages = wp_expand_stages();
""" % (len(stage1), len(stage2), len(r1), len(r2))
    body = "\n\n".join([
        _array("constexpr", "uint16_t", "kWpStage1Runs", r1, "%d", 40),
        _array("constexpr", "uint16_t", "kWpStage2Runs", r2, "%d", 40),
        _array("TCAMD_WP_TABLE_ATTR const", "uint32_t", "kWpEntries", entries, "0x%x", 14),
        _array("TCAMD_WP_TABLE_ATTR const", "uint32_t", "kWpExt", ext, "0x%x", 14),
    ])
    return head + body + tail


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--check", action="store_true", help="compare with the committed header instead of writing it")
    args = ap.parse_args()
    text = render()
    if args.check:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("up to date" if same else "csrc/kernels/wordpiece_table.h differs from a fresh run")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s (%d bytes)" % (os.path.relpath(OUT, REPO), len(text)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
