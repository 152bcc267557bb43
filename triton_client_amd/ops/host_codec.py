"""ctypes binding of libtcamd_host.so (BYTES pack / scan, baseline JPEG and PNG on the host, the compare rule,
the answer-span rule, the BERT tokenizer)."""
import ctypes
import os

import numpy as np

from . import dtypes

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libtcamd_host.so")


class JpegInfo(ctypes.Structure):
    """TcamdJpegInfo of csrc/host/jpeg.h: the image and the layout of its
    coefficient buffer (uint16 q[ncomp][64], then component c's ``bw[c] x
    bh[c]`` blocks of ``ny[c] * nx[c]`` int16 at ``coef_off[c]``).  ``h x w``
    is the decoded size: the source's at ``scale`` 1 (8 x 8 blocks), and
    ``ceil(H / scale) x ceil(W / scale)`` at 2, 4 and 8."""

    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ncomp", ctypes.c_int32), ("hs", ctypes.c_int32),
                ("vs", ctypes.c_int32), ("bw", ctypes.c_int32 * 3), ("bh", ctypes.c_int32 * 3),
                ("coef_off", ctypes.c_uint64 * 3), ("coef_bytes", ctypes.c_uint64), ("scale", ctypes.c_int32),
                ("ny", ctypes.c_int32 * 3), ("nx", ctypes.c_int32 * 3)]

    @property
    def shape(self):
        return (self.h, self.w, self.ncomp)

    @property
    def pixel_bytes(self):
        return self.h * self.w * self.ncomp


class PngInfo(ctypes.Structure):
    """TcamdPngInfo of csrc/host/png.h: the IHDR fields, ``channels`` of the
    uint8 output (1 or 3), the unfilter distance ``bpp``, ``row_bytes`` of a
    scanline without its filter byte, ``filtered_bytes`` that the IDAT stream
    inflates to, and the layout of the staged bytes K25 ``png_unfilter`` reads
    (``stage_bytes`` in all): the scanlines, the palette of colour type 3 at
    ``palette_off``, and for an image of more rows than a pass of K25 one
    scanline of scratch at ``line_off`` (0 = absent)."""

    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("depth", ctypes.c_int32), ("ctype", ctypes.c_int32),
                ("interlace", ctypes.c_int32), ("channels", ctypes.c_int32), ("bpp", ctypes.c_int32),
                ("row_bytes", ctypes.c_uint32), ("filtered_bytes", ctypes.c_uint64), ("pixel_bytes", ctypes.c_uint64),
                ("palette_off", ctypes.c_uint64), ("line_off", ctypes.c_uint64), ("stage_bytes", ctypes.c_uint64)]

    @property
    def shape(self):
        return (self.h, self.w, self.channels)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_KIND = {1: "unsupported PNG: ", 2: "malformed PNG: "}


def aligned_buffer(nbytes, align=16):
    """An uninitialised uint8 array of ``nbytes`` whose first byte is ``align``-byte aligned."""
    a = np.empty(nbytes + align, dtype=np.uint8)
    o = -a.ctypes.data % align
    return a[o:o + nbytes]


JPEG_SCALES = (1, 2, 4, 8)


def _check_scale(scale):
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or scale not in JPEG_SCALES:
        raise ValueError("jpeg scale must be 1, 2, 4 or 8, not %r" % (scale,))
    return int(scale)


_JPEG_KIND = {1: "unsupported JPEG: ", 2: "malformed JPEG: "}
JPEG_NOT_PACKABLE = 3  # TCAMD_JPEG_NOT_PACKABLE: no error, the host entropy decoder's turn


class HostCodec:
    def __init__(self, lib):
        self._lib = lib
        lib.tcamd_host_jpeg_parse.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(JpegInfo), ctypes.c_char_p,
                                         ctypes.c_int]
        lib.tcamd_host_jpeg_parse.restype = ctypes.c_int
        for fn in (lib.tcamd_host_jpeg_entropy_decode, lib.tcamd_host_jpeg_decode):
            fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p,
                           ctypes.c_int]
            fn.restype = ctypes.c_int
        lib.tcamd_host_jpeg_parse_scaled.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                     ctypes.POINTER(JpegInfo), ctypes.c_char_p, ctypes.c_int]
        lib.tcamd_host_jpeg_parse_scaled.restype = ctypes.c_int
        for fn in (lib.tcamd_host_jpeg_entropy_decode_scaled, lib.tcamd_host_jpeg_decode_scaled):
            fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                           ctypes.c_char_p, ctypes.c_int]
            fn.restype = ctypes.c_int
        lib.tcamd_host_jpeg_stream_bound.argtypes = [ctypes.c_uint64]
        lib.tcamd_host_jpeg_stream_bound.restype = ctypes.c_uint64
        lib.tcamd_host_jpeg_stream_pack.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                    ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(JpegInfo),
                                                    ctypes.c_char_p, ctypes.c_int]
        lib.tcamd_host_jpeg_stream_pack.restype = ctypes.c_int
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.tcamd_host_jpeg_huffman_emulate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, u32p, u32p]
        lib.tcamd_host_jpeg_huffman_emulate.restype = ctypes.c_int
        lib.tcamd_host_jpeg_stream_bound_wide.argtypes = [ctypes.c_uint64]
        lib.tcamd_host_jpeg_stream_bound_wide.restype = ctypes.c_uint64
        lib.tcamd_host_jpeg_stream_pack_wide.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p,
                                                         ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), u32p,
                                                         ctypes.POINTER(JpegInfo), ctypes.c_char_p, ctypes.c_int]
        lib.tcamd_host_jpeg_stream_pack_wide.restype = ctypes.c_int
        lib.tcamd_host_jpeg_huffman_wide_emulate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                             ctypes.c_uint32, u32p, u32p]
        lib.tcamd_host_jpeg_huffman_wide_emulate.restype = ctypes.c_int
        lib.tcamd_host_jpeg_huffman_wide_workspace.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
        lib.tcamd_host_jpeg_huffman_wide_workspace.restype = ctypes.c_uint64
        lib.tcamd_host_png_parse.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(PngInfo), ctypes.c_char_p,
                                             ctypes.c_int]
        lib.tcamd_host_png_parse.restype = ctypes.c_int
        for fn in (lib.tcamd_host_png_inflate, lib.tcamd_host_png_decode):
            fn.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p,
                           ctypes.c_int]
            fn.restype = ctypes.c_int
        lib.tcamd_host_png_unfilter.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(PngInfo), ctypes.c_void_p,
                                                ctypes.c_uint64]
        lib.tcamd_host_png_unfilter.restype = ctypes.c_int
        lib.tcamd_host_compare_expected.argtypes = [ctypes.POINTER(dtypes.ComparePair), ctypes.c_int, ctypes.c_double,
                                                    ctypes.c_double, ctypes.POINTER(dtypes.CompareRecord)]
        lib.tcamd_host_compare_expected.restype = ctypes.c_int
        lib.tcamd_host_qa_spans.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]
        lib.tcamd_host_qa_spans.restype = ctypes.c_int
        lib.tcamd_host_qa_spans_masked.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32,
                                                   ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.tcamd_host_qa_spans_masked.restype = ctypes.c_int
        lib.tcamd_host_qa_merge.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                            ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p]
        lib.tcamd_host_qa_merge.restype = ctypes.c_int
        wpw = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
               ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint64]
        wouts = [ctypes.c_int32] + [ctypes.c_void_p] * 8
        lib.tcamd_host_wordpiece_windows.argtypes = wpw + wouts
        lib.tcamd_host_wordpiece_windows.restype = ctypes.c_int
        lib.tcamd_host_wordpiece_windows_emulate.argtypes = wpw + [ctypes.c_void_p, ctypes.c_uint64] + wouts
        lib.tcamd_host_wordpiece_windows_emulate.restype = ctypes.c_int
        lib.tcamd_host_wordpiece_windows_workspace.argtypes = [ctypes.c_int32, ctypes.c_uint64]
        lib.tcamd_host_wordpiece_windows_workspace.restype = ctypes.c_uint64
        wp = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
              ctypes.c_void_p, ctypes.c_uint64]
        outs = [ctypes.c_void_p] * 6
        lib.tcamd_host_wordpiece_tokenize.argtypes = wp + outs
        lib.tcamd_host_wordpiece_tokenize.restype = ctypes.c_int
        lib.tcamd_host_wordpiece_emulate.argtypes = wp + [ctypes.c_void_p, ctypes.c_uint64] + outs
        lib.tcamd_host_wordpiece_emulate.restype = ctypes.c_int
        lib.tcamd_host_wordpiece_workspace.argtypes = [ctypes.c_int32, ctypes.c_uint64]
        lib.tcamd_host_wordpiece_workspace.restype = ctypes.c_uint64
        lib.tcamd_host_wordpiece_geometry.argtypes = [ctypes.POINTER(ctypes.c_int32)]
        lib.tcamd_host_wordpiece_geometry.restype = None
        lib.tcamd_host_wordpiece_fold.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        lib.tcamd_host_wordpiece_fold.restype = ctypes.c_int
        lib.tcamd_host_wordpiece_vocab_check.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        lib.tcamd_host_wordpiece_vocab_check.restype = ctypes.c_int
        lib.tcamd_host_pack_bytes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        lib.tcamd_host_pack_bytes.restype = ctypes.c_int
        lib.tcamd_host_count_bytes.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        lib.tcamd_host_count_bytes.restype = ctypes.c_int64
        lib.tcamd_host_scan_bytes.argtypes = [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
        ]
        lib.tcamd_host_scan_bytes.restype = ctypes.c_int64
        lib.tcamd_host_scan_bytes_prefix.argtypes = [
            ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
        ]
        lib.tcamd_host_scan_bytes_prefix.restype = ctypes.c_int64

    def pack_bytes(self, elems, lens):
        payload = b"".join(elems)
        lens = np.ascontiguousarray(lens, dtype="<u4")
        out = ctypes.create_string_buffer(len(payload) + 4 * len(elems))
        self._lib.tcamd_host_pack_bytes(payload, lens.ctypes.data, len(elems), out)
        return out.raw

    def scan_bytes(self, buf):
        arr = np.frombuffer(buf, dtype=np.uint8)
        ptr = arr.ctypes.data
        n = self._lib.tcamd_host_count_bytes(ptr, arr.size)
        if n < 0:
            raise ValueError("malformed BYTES tensor: element overruns buffer")
        offs = np.empty(n, dtype=np.uint64)
        lens = np.empty(n, dtype=np.uint32)
        self._lib.tcamd_host_scan_bytes(ptr, arr.size, offs.ctypes.data, lens.ctypes.data, n)
        return offs, lens


    def scan_prefix(self, arr, offs, lens, cap):
        """Index up to ``cap`` complete elements of the uint8 array ``arr`` (a
        prefix of a BYTES stream) into ``offs`` / ``lens``; returns (count,
        bytes consumed)."""
        consumed = ctypes.c_uint64(0)
        n = self._lib.tcamd_host_scan_bytes_prefix(arr.ctypes.data, arr.size, offs.ctypes.data, lens.ctypes.data,
                                                   cap, ctypes.byref(consumed))
        return int(n), int(consumed.value)


    # -- the compare rule (csrc/kernels/compare_math.h) ---------------------------------
    def compare_expected(self, pairs, atol=0.0, rtol=0.0):
        """K26 ``compare_expected`` on the host, field for field: ``pairs`` is up
        to 64 tuples ``(got, expected, datatype)`` of numpy arrays of equal size
        (any dtype of the datatype's width; only their bytes are read).  Returns
        one ``(mismatches, first_index, max_abs_diff, got_bits, expected_bits)``
        per pair, ``first_index`` ``dtypes.COMPARE_NO_INDEX`` when nothing
        mismatches."""
        keep, tab = [], []
        for got, exp, dt in pairs:
            g, e = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
            dtypes.code(dt)  # ValueError for a datatype the kernels do not know
            if g.nbytes != e.nbytes or g.nbytes % dtypes.SIZES[dt]:
                raise ValueError("compare_expected: got and expected must hold the same whole number of %s" % dt)
            keep.append((g, e))
            tab.append((g.ctypes.data, e.ctypes.data, g.nbytes // dtypes.SIZES[dt], dt))
        rec = (dtypes.CompareRecord * max(len(tab), 1))()
        if self._lib.tcamd_host_compare_expected(dtypes.compare_table(tab), len(tab), float(atol), float(rtol), rec):
            raise ValueError("compare_expected: a pointer, datatype or tolerance the rule refuses")
        return [rec[i].astuple() for i in range(len(tab))]

    # -- the answer-span rule (csrc/kernels/qa_span_math.h) ------------------------------
    def qa_spans_raw(self, start_ptr, end_ptr, logit_stride_bytes, mask_ptr, token_type_ptr, ids_stride_bytes, rows, S,
                     k_row_ptr, len_row_ptr, kmax, spans_ptr, scores_ptr, null_score_ptr):
        """``ops.hip.qa_spans`` on host addresses, argument for argument (no
        stream); ``ValueError`` for what the device entry refuses."""
        if self._lib.tcamd_host_qa_spans(start_ptr, end_ptr, int(logit_stride_bytes), mask_ptr, token_type_ptr,
                                         int(ids_stride_bytes), int(rows), int(S), k_row_ptr, len_row_ptr, int(kmax),
                                         spans_ptr, scores_ptr, null_score_ptr):
            raise ValueError("qa_spans: a size, pointer or stride the rule refuses")

    def qa_spans(self, start, end, attention_mask, token_type_ids, k_row, len_row, kmax=None):
        """K27 ``qa_spans`` on the host, bit for bit: ``start`` / ``end`` fp32
        ``[rows, S]``, ``attention_mask`` / ``token_type_ids`` int32 ``[rows, S]``,
        ``k_row`` / ``len_row`` int32 ``[rows]`` (the answers wanted and the
        longest answer of each row), ``kmax`` the ranks of the outputs (default:
        the largest ``k_row``, at least 1).  Returns ``(spans, scores,
        null_score)``: int32 ``[rows, kmax, 2]``, fp32 ``[rows, kmax]`` and fp32
        ``[rows]``.  Ranks past a row's candidates hold ``(-1, -1)`` and
        ``-FLT_MAX``; ranks past ``k_row[r]``, and everything of a row with
        ``k_row[r] < 1``, hold zeros (the routine does not write them)."""
        st = np.ascontiguousarray(start, dtype=np.float32)
        en = np.ascontiguousarray(end, dtype=np.float32)
        mk = np.ascontiguousarray(attention_mask, dtype=np.int32)
        tt = np.ascontiguousarray(token_type_ids, dtype=np.int32)
        if st.ndim != 2 or not (st.shape == en.shape == mk.shape == tt.shape):
            raise ValueError("qa_spans: the four inputs must be [rows, S] arrays of one shape")
        rows, S = st.shape
        k = np.ascontiguousarray(k_row, dtype=np.int32).reshape(-1)
        ln = np.ascontiguousarray(len_row, dtype=np.int32).reshape(-1)
        if k.size != rows or ln.size != rows:
            raise ValueError("qa_spans: k_row and len_row must have one entry per row")
        if kmax is None:
            kmax = max(1, int(k.max())) if rows else 1
        spans = np.zeros((rows, kmax, 2), dtype=np.int32)
        scores = np.zeros((rows, kmax), dtype=np.float32)
        null = np.zeros((max(rows, 1),), dtype=np.float32)
        one = np.zeros(1, dtype=np.int32)  # rows == 0: the entry still wants non-null pointers
        ptr = lambda a: a.ctypes.data if a.size else one.ctypes.data  # noqa: E731
        self.qa_spans_raw(ptr(st), ptr(en), S * 4, ptr(mk), ptr(tt), S * 4, rows, S, ptr(k), ptr(ln), kmax,
                          ptr(spans), ptr(scores), null.ctypes.data)
        return spans, scores, null[:rows]

    def qa_spans_masked(self, start, end, attention_mask, token_type_ids, start_mask, k_row, len_row, kmax=None):
        """K27 with a start mask on the host, bit for bit: :meth:`qa_spans`, and
        a span may start only where ``start_mask`` (int32 ``[rows, S]``) is at
        least 1."""
        st = np.ascontiguousarray(start, dtype=np.float32)
        en = np.ascontiguousarray(end, dtype=np.float32)
        mk = np.ascontiguousarray(attention_mask, dtype=np.int32)
        tt = np.ascontiguousarray(token_type_ids, dtype=np.int32)
        so = np.ascontiguousarray(start_mask, dtype=np.int32)
        if st.ndim != 2 or not (st.shape == en.shape == mk.shape == tt.shape == so.shape):
            raise ValueError("qa_spans_masked: the five inputs must be [rows, S] arrays of one shape")
        rows, S = st.shape
        k = np.ascontiguousarray(k_row, dtype=np.int32).reshape(-1)
        ln = np.ascontiguousarray(len_row, dtype=np.int32).reshape(-1)
        if k.size != rows or ln.size != rows:
            raise ValueError("qa_spans_masked: k_row and len_row must have one entry per row")
        if kmax is None:
            kmax = max(1, int(k.max())) if rows else 1
        spans = np.zeros((rows, kmax, 2), dtype=np.int32)
        scores = np.zeros((rows, kmax), dtype=np.float32)
        null = np.zeros((max(rows, 1),), dtype=np.float32)
        one = np.zeros(1, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a.size else one.ctypes.data  # noqa: E731
        if self._lib.tcamd_host_qa_spans_masked(ptr(st), ptr(en), S * 4, ptr(mk), ptr(tt), ptr(so), S * 4, rows, S,
                                                ptr(k), ptr(ln), int(kmax), ptr(spans), ptr(scores), null.ctypes.data):
            raise ValueError("qa_spans_masked: a size, pointer or stride the rule refuses")
        return spans, scores, null[:rows]

    def qa_merge(self, spans, scores, null_score, window_info, doc_info, k_doc, kmax=None):
        """K29 ``qa_merge`` on the host, bit for bit: ``spans`` int32 ``[rows,
        kmax, 2]``, ``scores`` fp32 ``[rows, kmax]`` and ``null_score`` fp32
        ``[rows]`` as :meth:`qa_spans_masked` returns them, ``window_info`` int32
        ``[rows, 4]`` and ``doc_info`` uint32 ``[docs, 4]`` as
        :meth:`wordpiece_windows` returns them, ``k_doc`` int32 ``[docs]``.
        Returns ``(spans [docs, kmax, 2], windows [docs, kmax], scores [docs,
        kmax], null_score [docs])``; ranks past ``k_doc[d]`` hold zeros."""
        sp = np.ascontiguousarray(spans, dtype=np.int32)
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        nu = np.ascontiguousarray(null_score, dtype=np.float32).reshape(-1)
        wi = np.ascontiguousarray(window_info, dtype=np.int32)
        di = np.ascontiguousarray(doc_info, dtype=np.uint32)
        if sp.ndim != 3 or sp.shape[2] != 2 or sc.shape != sp.shape[:2] or nu.size != sp.shape[0] \
                or wi.shape != (sp.shape[0], 4) or di.ndim != 2 or di.shape[1] != 4:
            raise ValueError("qa_merge: spans [rows, kmax, 2], scores [rows, kmax], null [rows], window_info "
                             "[rows, 4] and doc_info [docs, 4]")
        rows, kin = sc.shape
        docs = di.shape[0]
        k = np.ascontiguousarray(k_doc, dtype=np.int32).reshape(-1)
        if k.size != docs:
            raise ValueError("qa_merge: k_doc must have one entry per document")
        if kmax is None:
            kmax = kin
        if kmax != kin:
            raise ValueError("qa_merge: kmax is the ranks of the input lists")
        o_sp = np.zeros((docs, kmax, 2), dtype=np.int32)
        o_wn = np.zeros((docs, kmax), dtype=np.int32)
        o_sc = np.zeros((docs, kmax), dtype=np.float32)
        o_nu = np.zeros((max(docs, 1),), dtype=np.float32)
        one = np.zeros(4, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a.size else one.ctypes.data  # noqa: E731
        if self._lib.tcamd_host_qa_merge(ptr(sp), ptr(sc), ptr(nu), rows, ptr(wi), ptr(di), docs, ptr(k), int(kmax),
                                         ptr(o_sp), ptr(o_wn), ptr(o_sc), o_nu.ctypes.data):
            raise ValueError("qa_merge: a size or pointer the rule refuses")
        return o_sp, o_wn, o_sc, o_nu[:docs]

    # -- the BERT tokenizer (csrc/kernels/wordpiece_core.h) -------------------------------
    WORDPIECE_GEOMETRY = ("chunk", "block", "max_text_bytes", "max_word_chars", "max_rows", "max_chunks")

    def wordpiece_geometry(self):
        """``ops.hip.wordpiece_geometry`` without the device library."""
        g = (ctypes.c_int32 * 6)()
        self._lib.tcamd_host_wordpiece_geometry(g)
        return dict(zip(self.WORDPIECE_GEOMETRY, (int(x) for x in g)))

    def wordpiece_workspace(self, rows, text_bytes):
        """``ops.hip.wordpiece_workspace`` without the device library."""
        return int(self._lib.tcamd_host_wordpiece_workspace(int(rows), int(text_bytes)))

    def wordpiece_fold(self, cp):
        """What code point ``cp`` folds to: 0 to 3 words, each a code point with
        bit 30 set when it is a word of its own (punctuation, CJK), or one word
        with bit 31 for a space; ``[]`` for a dropped code point."""
        out = (ctypes.c_uint32 * 3)()
        n = self._lib.tcamd_host_wordpiece_fold(int(cp), out)
        if n < 0:
            raise ValueError("no code point %#x" % cp)
        return [int(out[i]) for i in range(n)]

    def wordpiece_tokenize(self, questions, contexts, vocab, max_query_length=64, S=384, emulate=False,
                           workspace_bytes=None):
        """K28 ``wordpiece_tokenize`` on the host, bit for bit: ``questions`` and
        ``contexts`` are bytes objects (UTF-8, unchecked), ``vocab`` a
        ``utils.wordpiece.Vocab``, ``max_query_length`` one int or one per row.
        Returns ``(ids, mask, type_ids, offsets, overflow, status)``: int32
        ``[rows, S]`` three times, int32 ``[rows, S, 2]`` (byte offsets into the
        context, context pieces only), int32 ``[rows]`` (context pieces that did
        not fit) and uint32 ``[rows]`` (0, or why the row is all zeros:
        ``utils.wordpiece.status_error``).  ``emulate`` runs the kernel's phases
        in the kernel's workspace layout instead of the front-to-back walk."""
        from triton_client_amd.utils import wordpiece as wp

        buf, table = wp.pack_texts(questions, contexts)
        rows = table.shape[0]
        mq = np.ascontiguousarray(np.broadcast_to(np.asarray(max_query_length, dtype=np.int32), (rows,)))
        image = np.ascontiguousarray(vocab.image, dtype=np.uint32)
        pad = max(rows, 1)
        ids, mask, tt = (np.zeros((pad, S), dtype=np.int32) for _ in range(3))
        offsets = np.zeros((pad, S, 2), dtype=np.int32)
        overflow, status = np.zeros(pad, dtype=np.int32), np.zeros(pad, dtype=np.uint32)
        text = buf if buf.size else np.zeros(4, dtype=np.uint8)
        tab = table if rows else np.zeros((1, 4), dtype=np.uint32)
        mqa = mq if rows else np.zeros(1, dtype=np.int32)
        head = (text.ctypes.data, int(buf.size), tab.ctypes.data, mqa.ctypes.data, rows, int(S), image.ctypes.data,
                int(image.size))
        outs = tuple(a.ctypes.data for a in (ids, mask, tt, offsets, overflow, status))
        if emulate:
            nbytes = self.wordpiece_workspace(rows, buf.size) if workspace_bytes is None else int(workspace_bytes)
            ws = np.zeros(max(nbytes // 4, 1), dtype=np.uint32)
            rc = self._lib.tcamd_host_wordpiece_emulate(*head, ws.ctypes.data, nbytes, *outs)
        else:
            rc = self._lib.tcamd_host_wordpiece_tokenize(*head, *outs)
        if rc:
            raise ValueError("wordpiece_tokenize: a size or pointer the rule refuses")
        return ids[:rows], mask[:rows], tt[:rows], offsets[:rows], overflow[:rows], status[:rows]

    def wordpiece_windows_workspace(self, docs, text_bytes):
        """``ops.hip.wordpiece_windows_workspace`` without the device library."""
        return int(self._lib.tcamd_host_wordpiece_windows_workspace(int(docs), int(text_bytes)))

    def wordpiece_windows(self, questions, contexts, vocab, max_query_length=64, doc_stride=128, max_windows=128, S=384,
                          out_rows=128, emulate=False, workspace_bytes=None):
        """K28w ``wordpiece_windows`` on the host, bit for bit: one document per
        question and context; ``max_query_length``, ``doc_stride`` and
        ``max_windows`` one int or one per document; ``out_rows`` the row
        capacity.  Returns ``(ids, mask, type_ids, start_mask, offsets,
        window_info, doc_info, n_rows)``: int32 ``[out_rows, S]`` four times,
        int32 ``[out_rows, S, 2]``, int32 ``[out_rows, 4]``, uint32 ``[docs, 4]``
        and an int (rule 8 of csrc/kernels/wordpiece_core.h).  ``emulate`` runs
        the kernel's phases in the kernel's workspace layout."""
        from triton_client_amd.utils import wordpiece as wp

        buf, table = wp.pack_texts(questions, contexts)
        docs = table.shape[0]
        per_doc = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.int32), (docs,)))  # noqa: E731
        mq, ds, mw = per_doc(max_query_length), per_doc(doc_stride), per_doc(max_windows)
        image = np.ascontiguousarray(vocab.image, dtype=np.uint32)
        cap = max(int(out_rows), 1)
        ids, mask, tt, sm = (np.zeros((cap, S), dtype=np.int32) for _ in range(4))
        offsets = np.zeros((cap, S, 2), dtype=np.int32)
        winfo = np.zeros((cap, 4), dtype=np.int32)
        dinfo = np.zeros((max(docs, 1), 4), dtype=np.uint32)
        n_rows = np.zeros(1, dtype=np.int32)
        text = buf if buf.size else np.zeros(4, dtype=np.uint8)
        tab = table if docs else np.zeros((1, 4), dtype=np.uint32)
        one = np.zeros(1, dtype=np.int32)
        head = (text.ctypes.data, int(buf.size), tab.ctypes.data) + tuple((a if docs else one).ctypes.data
                                                                          for a in (mq, ds, mw)) + \
            (docs, int(S), image.ctypes.data, int(image.size))
        outs = (int(out_rows),) + tuple(a.ctypes.data for a in (ids, mask, tt, sm, offsets, winfo, dinfo, n_rows))
        if emulate:
            nbytes = self.wordpiece_windows_workspace(docs, buf.size) if workspace_bytes is None \
                else int(workspace_bytes)
            ws = np.zeros(max(nbytes // 4, 1), dtype=np.uint32)
            rc = self._lib.tcamd_host_wordpiece_windows_emulate(*head, ws.ctypes.data, nbytes, *outs)
        else:
            rc = self._lib.tcamd_host_wordpiece_windows(*head, *outs)
        if rc:
            raise ValueError("wordpiece_windows: a size or pointer the rule refuses")
        return ids, mask, tt, sm, offsets, winfo, dinfo[:docs], int(n_rows[0])

    # -- baseline JPEG (csrc/host/jpeg.cc) ---------------------------------------------
    @staticmethod
    def _jpeg_check(rc, msg):
        if rc:
            raise ValueError(_JPEG_KIND.get(rc, "JPEG: ") + msg.value.decode())

    def jpeg_parse(self, blob, scale=1):
        """The :class:`JpegInfo` of a JPEG blob; ``ValueError`` ("unsupported
        JPEG: ..." / "malformed JPEG: ...") when it cannot be decoded.  With
        ``scale`` 2, 4 or 8 it describes the reduced-size decode: the scaled
        shape, each component's transform size and the compact buffer."""
        info = JpegInfo()
        msg = ctypes.create_string_buffer(96)
        if _check_scale(scale) == 1:
            rc = self._lib.tcamd_host_jpeg_parse(blob, len(blob), ctypes.byref(info), msg, len(msg))
        else:
            rc = self._lib.tcamd_host_jpeg_parse_scaled(blob, len(blob), scale, ctypes.byref(info), msg, len(msg))
        self._jpeg_check(rc, msg)
        return info

    def jpeg_entropy_decode(self, blob, out, scale=1):
        """Huffman-decode ``blob`` into the uint8 array ``out`` (at least
        ``coef_bytes`` of its parse at ``scale``, 16-byte aligned):
        quantisation tables, then the de-zigzagged int16 coefficients, not
        dequantised.  At ``scale`` 2, 4 or 8 only the coefficients the reduced
        transform uses are stored; the stream is walked and checked in full."""
        msg = ctypes.create_string_buffer(96)
        if _check_scale(scale) == 1:
            rc = self._lib.tcamd_host_jpeg_entropy_decode(blob, len(blob), out.ctypes.data, out.size, msg, len(msg))
        else:
            rc = self._lib.tcamd_host_jpeg_entropy_decode_scaled(blob, len(blob), scale, out.ctypes.data, out.size,
                                                                 msg, len(msg))
        self._jpeg_check(rc, msg)

    def jpeg_decode(self, blob, scale=1):
        """Blob -> uint8 [H, W, 1 or 3], entirely on the host; at ``scale`` 2, 4
        or 8 decoded in the DCT domain to ``ceil(H / scale) x ceil(W / scale)``."""
        info = self.jpeg_parse(blob, scale)
        out = np.empty(info.shape, dtype=np.uint8)
        msg = ctypes.create_string_buffer(96)
        if scale == 1:
            rc = self._lib.tcamd_host_jpeg_decode(blob, len(blob), out.ctypes.data, out.size, msg, len(msg))
        else:
            rc = self._lib.tcamd_host_jpeg_decode_scaled(blob, len(blob), scale, out.ctypes.data, out.size, msg,
                                                         len(msg))
        self._jpeg_check(rc, msg)
        return out

    # -- the stream buffer of K23 jpeg_huffman (csrc/kernels/jpeg_huff_core.h) ----------
    def jpeg_stream_bound(self, nbytes):
        """A capacity that holds the stream buffer of every packable blob of ``nbytes``."""
        return int(self._lib.tcamd_host_jpeg_stream_bound(int(nbytes)))

    def jpeg_stream_pack(self, blob, out):
        """Pack the scan of ``blob`` into the uint8 array ``out`` (16-byte
        aligned, :func:`aligned_buffer`; anything else is not packable) as the
        stream buffer ``ops.hip.jpeg_huffman`` reads: header, quantisation and Huffman tables, segment table, the entropy-coded bytes
        without stuffing and restart markers.  Returns ``(info, used)``, the
        parse and the bytes written, or ``(info, None)`` when the blob is not
        packable (anything unusual about its restart markers or what follows
        the scan, a scan above the kernel's 2048 x 128 bytes, or ``out`` too
        small): the caller then takes :meth:`jpeg_entropy_decode`, which gives
        the answer or the error.  A blob that does not parse raises as
        :meth:`jpeg_parse` does."""
        info = JpegInfo()
        used = ctypes.c_uint64(0)
        msg = ctypes.create_string_buffer(96)
        rc = self._lib.tcamd_host_jpeg_stream_pack(blob, len(blob), out.ctypes.data, out.size, ctypes.byref(used),
                                                   ctypes.byref(info), msg, len(msg))
        if rc == JPEG_NOT_PACKABLE:
            return info, None
        self._jpeg_check(rc, msg)
        return info, int(used.value)

    def jpeg_huffman_emulate(self, stream, out):
        """K23 ``jpeg_huffman`` run on the host, thread by thread and phase by
        phase from the kernel's own header: the uint8 array ``stream`` (a packed
        stream buffer) -> coefficients in ``out`` (``coef_bytes`` of the parse,
        16-byte aligned).  Returns ``(status, rounds)``: the kernel's status
        word (0 = the coefficients are good) and the sync rounds it took."""
        status, rounds = ctypes.c_uint32(0), ctypes.c_uint32(0)
        if self._lib.tcamd_host_jpeg_huffman_emulate(stream.ctypes.data, out.ctypes.data, out.size,
                                                     ctypes.byref(status), ctypes.byref(rounds)):
            raise MemoryError("jpeg_huffman_emulate")
        return int(status.value), int(rounds.value)

    # -- the stream buffer of the K24 jpeg_huffman_wide kernels (csrc/kernels/jpeg_huff_wide_core.h)
    def jpeg_stream_bound_wide(self, nbytes):
        """A capacity that holds the wide stream buffer of every packable blob of ``nbytes``."""
        return int(self._lib.tcamd_host_jpeg_stream_bound_wide(int(nbytes)))

    def jpeg_stream_pack_wide(self, blob, out, scale=1):
        """:meth:`jpeg_stream_pack` for ``ops.hip.jpeg_huffman_wide``: the same
        one-pass pack under another magic word, with ``scale`` (1, 2, 4 or 8)
        in the header and a ceiling of 32 MiB of scan data instead of 256 KiB.
        Returns ``(info, used, nsub)``: the parse at ``scale``, the bytes
        written and the scan's subsequences (they size the kernel's grid and
        workspace), or ``(info, None, None)`` when the blob is not packable."""
        info = JpegInfo()
        used, nsub = ctypes.c_uint64(0), ctypes.c_uint32(0)
        msg = ctypes.create_string_buffer(96)
        rc = self._lib.tcamd_host_jpeg_stream_pack_wide(blob, len(blob), _check_scale(scale), out.ctypes.data, out.size,
                                                        ctypes.byref(used), ctypes.byref(nsub), ctypes.byref(info),
                                                        msg, len(msg))
        if rc == JPEG_NOT_PACKABLE:
            return info, None, None
        self._jpeg_check(rc, msg)
        return info, int(used.value), int(nsub.value)

    def jpeg_huffman_wide_emulate(self, stream, out, chunk_subs=0):
        """The K24 launch sequence run on the host, launch by launch, workgroup
        by workgroup and thread by thread from the kernels' own header: the
        uint8 array ``stream`` (a wide stream buffer) -> coefficients in
        ``out`` (``coef_bytes`` of the parse at the stream's scale, 16-byte
        aligned), in chunks of ``chunk_subs`` subsequences (a power of two up
        to 1024; 0 = the default 1024).  Returns ``(status, changed)``: the
        status word (0 = the coefficients are good) and the inter-chunk
        launches in which a chunk took a new entry."""
        status, changed = ctypes.c_uint32(0), ctypes.c_uint32(0)
        if self._lib.tcamd_host_jpeg_huffman_wide_emulate(stream.ctypes.data, out.ctypes.data, out.size,
                                                          int(chunk_subs), ctypes.byref(status),
                                                          ctypes.byref(changed)):
            raise MemoryError("jpeg_huffman_wide_emulate")
        return int(status.value), int(changed.value)

    def jpeg_huffman_wide_workspace(self, nsubs, chunk_subs=0):
        """``ops.hip.jpeg_huffman_wide_workspace`` without the device library:
        the bytes of workspace a K24 call over images of ``nsubs``
        subsequences needs at ``chunk_subs`` (0 = the default 1024)."""
        cs = int(chunk_subs) or 1024
        return int(self._lib.tcamd_host_jpeg_huffman_wide_workspace(sum(int(n) for n in nsubs),
                                                                    sum(-(-int(n) // cs) for n in nsubs)))

    # -- PNG (csrc/host/png.cc) ----------------------------------------------------------
    @staticmethod
    def _png_check(rc, msg):
        if rc:
            raise ValueError(_PNG_KIND.get(rc, "PNG: ") + msg.value.decode())

    def png_parse(self, blob):
        """The :class:`PngInfo` of a PNG blob, from its chunk headers alone
        (nothing is inflated); ``ValueError`` ("unsupported PNG: ..." /
        "malformed PNG: ...") when it cannot be decoded."""
        info = PngInfo()
        msg = ctypes.create_string_buffer(96)
        self._png_check(self._lib.tcamd_host_png_parse(blob, len(blob), ctypes.byref(info), msg, len(msg)), msg)
        return info

    def png_inflate(self, blob, out):
        """Inflate the IDAT stream of a non-interlaced ``blob`` straight into
        the uint8 array ``out`` (at least ``stage_bytes`` of its parse), with no
        intermediate copy: the filtered scanlines, then for colour type 3 the
        palette (256 x 3 bytes, zero past the end of PLTE) at the next 16-byte
        boundary: the staged bytes ``ops.hip.png_unfilter`` reads.  Checks the
        CRC of the IDAT chunks, the inflated length and the ``h`` filter-type
        bytes."""
        msg = ctypes.create_string_buffer(96)
        self._png_check(self._lib.tcamd_host_png_inflate(blob, len(blob), out.ctypes.data, out.size, msg, len(msg)), msg)

    def png_unfilter(self, staged, info):
        """K25 ``png_unfilter`` on the host, bitwise: the staged bytes of
        :meth:`png_inflate` (a uint8 array) -> uint8 [h, w, 1 or 3]."""
        out = np.empty(info.shape, dtype=np.uint8)
        staged = np.ascontiguousarray(staged, dtype=np.uint8)
        if self._lib.tcamd_host_png_unfilter(staged.ctypes.data, staged.size, ctypes.byref(info), out.ctypes.data,
                                             out.size):
            raise ValueError("png_unfilter: the staged bytes and the parse do not belong together")
        return out

    def png_decode(self, blob):
        """Blob -> uint8 [H, W, 1 or 3], entirely on the host, Adam7 included."""
        info = self.png_parse(blob)
        out = np.empty(info.shape, dtype=np.uint8)
        msg = ctypes.create_string_buffer(96)
        self._png_check(self._lib.tcamd_host_png_decode(blob, len(blob), out.ctypes.data, out.size, msg, len(msg)), msg)
        return out


_INSTANCE = None


def load():
    global _INSTANCE
    if _INSTANCE is None:
        _INSTANCE = HostCodec(ctypes.CDLL(_PATH))
    return _INSTANCE
