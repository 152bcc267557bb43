// The body of the K12 attention kernels (csrc/kernels/bert.hip), as a function
// of a row geometry.  Not a header in the usual sense: bert.hip includes it
// INSIDE the body of each of its two attention kernels, K12 and K12v, so that
// both are compiled from one text and K12's generated code is exactly what
// it was when this text stood in its kernel.  (The same text as an inlined
// __device__ function template computes the same thing but does not give the
// same code: the inliner's clone reorders use lists, and the vectoriser and
// the register allocator then settle differently.  tools/isa_diff.py on
// attention_kernel<true / false> is the check, profiles/r22_bert_packed.md
// has the result.)
//
// The including kernel provides
//   qkv, mask, out, S, heads, scale, qkv_bias   K12's parameters; S = the number
//                    of keys the row stages, a multiple of 64 and <= 384
//   MASKED, PACKED   compile-time bools
//   TC_ATTN_ROW_GEOMETRY   declarations of ``head`` and ``len`` (the row's head
//                    and its valid length; K12: len = S) at the point where
//                    K12 always computed its sequence and head
//   TC_ATTN_ROW_TOK0       the row's first token, a size_t expression
//
// Barriers: there is exactly one, the __syncthreads() behind the staging, and
// every wave of a block that comes here reaches it.  Nothing before it
// returns or branches around it: the staging loop, the key-bias loop and the
// query loads are plain loops and predicated loads.  With PACKED a wave whose
// 32 queries all lie at or past ``len`` skips its query loads (a wave-uniform
// branch that rejoins before the barrier), stages its share of K / V like
// every other wave, passes the barrier and only then returns; a block with
// no live wave at all (an empty row, or a query split past the row's end)
// never comes here: K12v's kernel returns first, on a condition that is
// uniform over the block.
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_a[];
  uint16_t* Ks = reinterpret_cast<uint16_t*>(lds_a);
  uint16_t* Vs = Ks + S * kAD;
  float* kb = reinterpret_cast<float*>(Vs + S * kAD);  // per-key log2-domain bias
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthr = blockDim.x;
  TC_ATTN_ROW_GEOMETRY
  const int HD = heads * kAD, ld = 3 * HD;
  const uint16_t* base = qkv + TC_ATTN_ROW_TOK0 * ld + head * kAD;
  constexpr float kLog2e = 1.4426950408889634f;

  // ---- stage K and V rows (128 B each) by LDS-DMA (round 6) ----
  // Both row-major, 16-B chunks XOR-swizzled on the SOURCE address (the DMA
  // writes lane-linear: one wave instruction = 8 rows), every instruction of
  // the block in flight at once and one wait.  K chunk c of key k sits at
  // c ^ ((k >> 1) & 7) (conflict-free b128 reads by 16 consecutive keys);
  // V chunk c at c ^ (((k >> 1) & 1) << 2), which makes the transposing
  // ds_read_b64_tr_b16 reads of the PV operand conflict-free.  (Round 5
  // staged with per-thread 16-B loads and transposed V by 4-byte LDS writes:
  // ~25 of 83 us at bs64 and half of bs1's 11 us went to that staging,
  // profiles/r6_k12/.)
  {
    const int nw = nthr >> 6, nrb = S >> 3;  // waves, 8-row blocks per operand
    const int r8 = lane >> 3, cs = lane & 7;
    for (int j = wave; j < 2 * nrb; j += nw) {
      const bool isv = j >= nrb;
      const int row = 8 * (isv ? j - nrb : j) + r8;
      const int c = isv ? cs ^ (((row >> 1) & 1) << 2) : cs ^ ((row >> 1) & 7);
      // packed: a key at or past len is the row's own last token (finite, and
      // never another row's or a pad token's); its bias below masks it
      const int srow = PACKED ? min(row, len - 1) : row;
      const uint16_t* src = base + (size_t)srow * ld + (isv ? 2 * HD : HD) + 8 * c;
      uint8_t* dst = lds_a + (isv ? S * 128 : 0) + (j - (isv ? nrb : 0)) * 1024;
      __builtin_amdgcn_global_load_lds((const void*)src, (void*)dst, 16, 0, 0);
    }
  }
  if (MASKED)
    for (int k = tid; k < S; k += nthr)
      kb[k] = (PACKED ? k >= len : mask[TC_ATTN_ROW_TOK0 + k] == 0) ? -10000.0f * kLog2e : 0.0f;

  // ---- this wave's queries: Q^T fragments (B operand: lane col = query) ----
  const int col = lane & 31, h = lane >> 5;
  const int q = 32 * (blockIdx.y * (nthr >> 6) + wave) + col;
  // packed: a wave with no query below len is dead (no loads, MFMAs or
  // stores; it leaves behind the barrier); a query at or past len in a live
  // wave is loaded from the row's last token and never stored
  const bool live = !PACKED || q - col < len;
  const int qsrc = PACKED ? min(q, len - 1) : q;
  v4u qf[4];
  if (PACKED && !live) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = v4u{0u, 0u, 0u, 0u};
  } else {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const v4u*>(base + (size_t)qsrc * ld + 16 * kk + 8 * h);
  }
  if (qkv_bias) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const v4u bq = *reinterpret_cast<const v4u*>(qkv_bias + head * kAD + 16 * kk + 8 * h);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float a0 = __uint_as_float(qf[kk][j] << 16) + __uint_as_float(bq[j] << 16);
        const float a1 = __uint_as_float(qf[kk][j] & 0xffff0000u) + __uint_as_float(bq[j] & 0xffff0000u);
        qf[kk][j] = pack2(a0, a1);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's K / V DMAs landed
  __syncthreads();                                   // ... and every other wave's
  if (PACKED && !live) return;  // wave-uniform, behind the kernel's only barrier

  const float sl2 = scale * kLog2e;
  float m_run = -1.0e30f, l_part = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[r][e] = 0.f;

  // Chunk classes (round 6).  A key-padding mask is a run of valid keys, so
  // most 64-key chunks are all valid or all padded: an all-valid chunk takes
  // the unmasked math (no bias add, one FMA per score into the exponent), an
  // all-padded chunk is skipped -- exactly: behind any valid key its scores
  // are exp2(<= -14000) = 0 in fp32, and if it comes first the first valid
  // chunk's rescale zeroes it.  Only a sequence with no valid key at all runs
  // every chunk masked (softmax over the padded scores, as torch does).
  const int nch = S / 64;
  uint32_t todo = (1u << nch) - 1u, full = todo;
  if constexpr (PACKED) {
    // a packed row's keys are a prefix: len / 64 all-valid chunks, then at
    // most one partial chunk (it holds a valid key, so no chunk is all padded)
    full = (1u << (len >> 6)) - 1u;
  } else if constexpr (MASKED) {
    full = 0u;
    uint32_t empty = 0u;
    for (int c = 0; c < nch; ++c) {
      const uint64_t v = __ballot(kb[64 * c + lane] == 0.0f);
      if (v == ~0ull) full |= 1u << c;
      if (v == 0ull) empty |= 1u << c;
    }
    if (empty != todo) todo &= ~empty;
  }

  // transposed V reads: lane 4 q4 + p4 of 16-lane group g supplies row (key)
  // 4 h + q4 of the 16-key step, dims 32 rd + 16 (g & 1) + 4 p4 .. + 3 (8 B of
  // chunk 4 rd + 2 (g & 1) + p4 / 2, swizzled by its key -- bit 1 of the key
  // is bit 1 of q4, the other terms are multiples of 4)
  const int q4 = (lane >> 2) & 3, p4 = lane & 3, g1 = (lane >> 4) & 1;
  const int vch = 2 * g1 + (p4 >> 1);
  const uint8_t* vbase = lds_a + S * 128 + (4 * h + q4) * 128 + ((vch ^ (((q4 >> 1) & 1) << 2)) << 4) + 8 * (p4 & 1);
  const int vrd = ((4 ^ (((q4 >> 1) & 1) << 2)) - (((q4 >> 1) & 1) << 2)) << 4;  // rd = 1: chunk + 4, swizzled
  // S^T for keys [c0, c0 + 64): two 32-key row blocks; lane (query, h) holds
  // keys 32 rb + 8 g + 4 h + e
  auto qk = [&](f32x16 (&st)[2], int c0) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[rb][e] = 0.f;
      const int key = c0 + 32 * rb + col;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const v4u kf = *reinterpret_cast<const v4u*>(Ks + key * kAD + 8 * ((2 * kk + h) ^ ((key >> 1) & 7)));
        st[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf8(kf), as_bf8(qf[kk]), st[rb], 0, 0, 0);
      }
    }
  };
  // online softmax of one chunk's scores and O^T += V^T P^T.  masked: x = s
  // scale log2e + bias, max and exp2(x - m) on x; unmasked (or an all-valid
  // chunk): max on the raw scores (scale > 0 commutes with max) and p =
  // exp2(s c - m c) as one FMA per score
  auto soft_pv = [&](f32x16 (&st)[2], int c0, auto bias_tag) {
    constexpr bool bias_chunk = decltype(bias_tag)::value;
    float mx = -1.0e30f;
    if constexpr (bias_chunk) {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bb = *reinterpret_cast<const f32x4*>(kb + c0 + 32 * rb + 8 * g + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = st[rb][4 * g + e] * sl2 + bb[e];
            st[rb][4 * g + e] = x;
            mx = fmaxf(mx, x);
          }
        }
    } else {
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, st[rb][e]);
      mx *= sl2;
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    m_run = m_new;
    f32x2 ls2 = f32x2{0.f, 0.f};
    v4u pf[4];  // P^T fragments per 16-key step: keys 16 kk2 + {4h..4h+3, 8+4h..8+4h+3}
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float pv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          pv[e] = bias_chunk ? __builtin_amdgcn_exp2f(st[rb][4 * g + e] - m_new)
                             : __builtin_amdgcn_exp2f(__builtin_fmaf(st[rb][4 * g + e], sl2, -m_new));
        ls2 += f32x2{pv[0], pv[1]} + f32x2{pv[2], pv[3]};
        const int kk2 = 2 * rb + (g >> 1), half = g & 1;
        pf[kk2][2 * half] = pack2(pv[0], pv[1]);
        pf[kk2][2 * half + 1] = pack2(pv[2], pv[3]);
      }
    const float ls = ls2[0] + ls2[1];
    l_part = l_part * alpha + ls;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[r][e] *= alpha;
    // O^T += V^T P^T: A = V^T rows (dims 32 rd + col), keys in the permuted
    // order, read TRANSPOSED from the row-major V image: ds_read_b64_tr_b16
    // gives lane i of a 16-lane group column i (= its dim) of 4 key rows
#pragma unroll
    for (int kk2 = 0; kk2 < 4; ++kk2)
#pragma unroll
      for (int rd = 0; rd < 2; ++rd) {
        const uint8_t* vr = vbase + (c0 + 16 * kk2) * 128 + rd * vrd;
        const v2u a0 = __builtin_bit_cast(v2u, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                                   (__attribute__((address_space(3))) v4s*)(vr)));
        const v2u a1 = __builtin_bit_cast(v2u, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                                   (__attribute__((address_space(3))) v4s*)(vr + 8 * 128)));
        const v4u af = v4u{a0[0], a0[1], a1[0], a1[1]};
        o[rd] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf8(af), as_bf8(pf[kk2]), o[rd], 0, 0, 0);
      }
  };
  // all-valid chunks first (unmasked math), then the partial ones (masked
  // math): the online softmax does not depend on the chunk order, and each
  // loop keeps one compile-time path (a per-chunk branch inside the softmax
  // cost registers and 10 % on the masked kernel, profiles/r6_k12.md)
  f32x16 st[2];
  for (uint32_t f = todo & full; f; f &= f - 1u) {
    const int c0 = 64 * __builtin_ctz(f);
    qk(st, c0);
    soft_pv(st, c0, std::false_type{});
  }
  if constexpr (MASKED)
    for (uint32_t m = todo & ~full; m; m &= m - 1u) {
      const int c0 = 64 * __builtin_ctz(m);
      qk(st, c0);
      soft_pv(st, c0, std::true_type{});
    }
  const float inv = 1.0f / (l_part + __shfl_xor(l_part, 32, 64));
  if (PACKED && q >= len) return;  // behind the last cross-lane step
  uint16_t* orow = out + (TC_ATTN_ROW_TOK0 + q) * HD + head * kAD;
#pragma unroll
  for (int rd = 0; rd < 2; ++rd)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = 32 * rd + 8 * g + 4 * h;
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if (qkv_bias) {
        const v2u b2 = *reinterpret_cast<const v2u*>(qkv_bias + 2 * HD + head * kAD + d);
        bv[0] = __uint_as_float(b2[0] << 16);
        bv[1] = __uint_as_float(b2[0] & 0xffff0000u);
        bv[2] = __uint_as_float(b2[1] << 16);
        bv[3] = __uint_as_float(b2[1] & 0xffff0000u);
      }
      *reinterpret_cast<v2u*>(orow + d) = v2u{pack2(o[rd][4 * g] * inv + bv[0], o[rd][4 * g + 1] * inv + bv[1]),
                                             pack2(o[rd][4 * g + 2] * inv + bv[2], o[rd][4 * g + 3] * inv + bv[3])};
    }
