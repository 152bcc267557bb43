// The body of the fp32-parity attention kernels (csrc/kernels/bert.hip), as a
// function of a row geometry.  Not a header in the usual sense: bert.hip
// includes it INSIDE the body of K12x (attention_x3_kernel<NW>) and of K12xv
// (attention_x3_packed_kernel<NW>), so that both are compiled from one text and
// K12x's generated code is exactly what it was when this text stood in its
// kernel -- the technique of kernels/bert_attention_row.h, for the reasons
// given there (an inlined function template computes the same thing but does
// not give the same code; tools/isa_diff.py on attention_x3_kernel<4 / 8> is
// the check, profiles/r23_bert_fp32_packed.md has the result).
//
// The including kernel provides
//   qkv, mask, out, out3, S, heads, scale   K12x's parameters (K12xv: mask null
//                    and S any value; with PACKED neither is used)
//   NW, PACKED       compile-time: waves per block, packed rows
//   TC_ATTN_X3_GEOMETRY   declarations of ``seq``, ``h`` (the row and its head)
//                    and ``len`` (its valid length; K12x: S, unused) at the
//                    point where K12x always computed its sequence and head
//   TC_ATTN_X3_TOK0       the row's first token, a size_t expression
//
// Barriers: one behind the first chunk's staging and one at the end of every
// chunk, all at the top level of the chunk loop, whose trip count
// ceil(len / 64) (K12x: S / 64) is uniform over the block.  The staging is
// cooperative -- every thread of the block loads and stores its share of each
// chunk's K, V and key bias -- so with PACKED no wave leaves before the loop
// ends, whatever its queries: a wave whose 16 queries all lie at or past
// ``len`` skips the chunk's MFMAs and softmax (a wave-uniform branch that
// rejoins before the staging stores and the barrier) and stores nothing, and
// a query at or past ``len`` in a live wave is loaded from the row's last
// token and never stored.  A block with no live wave at all (an empty row, a
// row that does not fit, a query block starting at or past len) never comes
// here: K12xv's kernel returns first, on conditions uniform over the block.
  extern __shared__ __attribute__((aligned(16))) uint8_t ldsa[];
  // per buffer: K hi [64 keys][kXR] | K lo | V^T hi [64 d][kXR] | V^T lo | key bias [64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  TC_ATTN_X3_GEOMETRY
  const int H = heads * 64, ld = 3 * H;
  const float* const base = qkv + TC_ATTN_X3_TOK0 * ld + h * 64;
  const int g = lane >> 4, c = lane & 15;
  const int q = blockIdx.y * (16 * NW) + wave * 16 + c;  // this lane's query
  const bool live = !PACKED || q - c < len;              // wave-uniform
  const int qsrc = PACKED ? min(q, len - 1) : q;

  // Q^T operand, pre-scaled (1/8: exact), d = 32 ks + 8 g .. +8
  v4u qh[2], ql[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const float4 a = *reinterpret_cast<const float4*>(base + (size_t)qsrc * ld + 32 * ks + 8 * g);
    const float4 b = *reinterpret_cast<const float4*>(base + (size_t)qsrc * ld + 32 * ks + 8 * g + 4);
    uint32_t hh[4], ll[4];
    split_pk(a.x * scale, a.y * scale, hh[0], ll[0]);
    split_pk(a.z * scale, a.w * scale, hh[1], ll[1]);
    split_pk(b.x * scale, b.y * scale, hh[2], ll[2]);
    split_pk(b.z * scale, b.w * scale, hh[3], ll[3]);
    qh[ks] = v4u{hh[0], hh[1], hh[2], hh[3]};
    ql[ks] = v4u{ll[0], ll[1], ll[2], ll[3]};
  }
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // staging of one 64-key chunk, split so that its global loads are in
  // flight during the previous chunk's math: K row-major (thread -> key, 4
  // head dims), V transposed (thread -> key pair, 4 head dims: 4-B words of
  // two keys, a wave's 32 key pairs one contiguous 128-B run per V^T row).
  // packed: a key at or past len is the row's own last token (finite, and
  // never another row's or a pad token's), each key of a V pair clamped on its
  // own; its -10000 bias masks it
  constexpr int KIT = 1024 / (64 * NW), VIT = 512 / (64 * NW);
  float4 kr[KIT], va[VIT], vb[VIT];
  float mkb = 0.f;
  auto stage_load = [&](int c0) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = it * 64 * NW + tid, key = i >> 4, d4 = (i & 15) * 4;
      kr[it] = *reinterpret_cast<const float4*>(base + (size_t)(PACKED ? min(c0 + key, len - 1) : c0 + key) * ld + H + d4);
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int u = it * 64 * NW + tid, kp = u & 31, d4 = (u >> 5) * 4;
      const float* r0 = base + (size_t)(PACKED ? min(c0 + 2 * kp, len - 1) : c0 + 2 * kp) * ld + 2 * H + d4;
      va[it] = *reinterpret_cast<const float4*>(r0);
      vb[it] = *reinterpret_cast<const float4*>(PACKED ? base + (size_t)min(c0 + 2 * kp + 1, len - 1) * ld + 2 * H + d4
                                                       : r0 + ld);
    }
    if (tid < 64) mkb = (PACKED ? c0 + tid >= len : (mask && mask[seq * S + c0 + tid] == 0)) ? -10000.f : 0.f;
  };
  auto stage_store = [&](uint8_t* buf) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int i = it * 64 * NW + tid, key = i >> 4, d4 = (i & 15) * 4;
      uint32_t h0, l0, h1, l1;
      split_pk(kr[it].x, kr[it].y, h0, l0);
      split_pk(kr[it].z, kr[it].w, h1, l1);
      *reinterpret_cast<uint2*>(buf + key * kXR + d4 * 2) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(buf + 64 * kXR + key * kXR + d4 * 2) = make_uint2(l0, l1);
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int u = it * 64 * NW + tid, kp = u & 31, d4 = (u >> 5) * 4;
      const float a[4] = {va[it].x, va[it].y, va[it].z, va[it].w}, b[4] = {vb[it].x, vb[it].y, vb[it].z, vb[it].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        uint32_t hh, ll;
        split_pk(a[j], b[j], hh, ll);
        *reinterpret_cast<uint32_t*>(buf + 128 * kXR + (d4 + j) * kXR + 4 * kp) = hh;
        *reinterpret_cast<uint32_t*>(buf + 192 * kXR + (d4 + j) * kXR + 4 * kp) = ll;
      }
    }
    if (tid < 64) reinterpret_cast<float*>(buf + 256 * kXR)[tid] = mkb;
  };
  stage_load(0);
  stage_store(ldsa);
  __syncthreads();
  const int nch = PACKED ? (len + 63) >> 6 : S / 64;
  for (int ci = 0; ci < nch; ++ci) {
    uint8_t* const kh = ldsa + (ci & 1) * kBufAX;  // K lo follows at kh + 64 * kXR
    uint8_t* const vth = kh + 128 * kXR;
    uint8_t* const vtl = kh + 192 * kXR;
    const float* const kb = reinterpret_cast<const float*>(kh + 256 * kXR);
    if (ci + 1 < nch) stage_load(64 * (ci + 1));

    if (!PACKED || live) {
    // S^T tiles [16 keys][16 queries]
    f32x4 st[4];
    float mx = m;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const uint8_t* ar = kh + (kt * 16 + c) * kXR + (32 * ks + 8 * g) * 2;
        st[kt] = mma_x3(*reinterpret_cast<const v4u*>(ar), *reinterpret_cast<const v4u*>(ar + 64 * kXR), qh[ks],
                        ql[ks], st[kt]);
      }
      const f32x4 kbv = *reinterpret_cast<const f32x4*>(kb + kt * 16 + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        st[kt][e] += kbv[e];
        mx = fmaxf(mx, st[kt][e]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float corr = __expf(m - mx);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        st[kt][e] = __expf(st[kt][e] - mx);
        sum += st[kt][e];
      }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    l = l * corr + sum;
    m = mx;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= corr;
    // O^T += V^T P^T over the chunk's two 32-key steps
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint32_t ph[4], pl[4];
      split_pk(st[2 * ks][0], st[2 * ks][1], ph[0], pl[0]);
      split_pk(st[2 * ks][2], st[2 * ks][3], ph[1], pl[1]);
      split_pk(st[2 * ks + 1][0], st[2 * ks + 1][1], ph[2], pl[2]);
      split_pk(st[2 * ks + 1][2], st[2 * ks + 1][3], ph[3], pl[3]);
      const v4u pbh = v4u{ph[0], ph[1], ph[2], ph[3]}, pbl = v4u{pl[0], pl[1], pl[2], pl[3]};
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int off = (dt * 16 + c) * kXR + (ks * 32 + 4 * g) * 2;
        const uint2 a0 = *reinterpret_cast<const uint2*>(vth + off), a1 = *reinterpret_cast<const uint2*>(vth + off + 32);
        const uint2 b0 = *reinterpret_cast<const uint2*>(vtl + off), b1 = *reinterpret_cast<const uint2*>(vtl + off + 32);
        o[dt] = mma_x3(v4u{a0.x, a0.y, a1.x, a1.y}, v4u{b0.x, b0.y, b1.x, b1.y}, pbh, pbl, o[dt]);
      }
    }
    }
    // chunk ci + 1 into the other buffer (read last in iteration ci - 1, which
    // every wave left behind the previous barrier)
    if (ci + 1 < nch) stage_store(ldsa + ((ci + 1) & 1) * kBufAX);
    __syncthreads();
  }
  if (PACKED && q >= len) return;  // behind the last barrier and the last cross-lane step
  const float inv = 1.f / l;
  if (out3) {
    uint16_t* const op = out3 + (TC_ATTN_X3_TOK0 + q) * 3 * H + h * 64 + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      f32x4 r = o[dt] * inv;
      // the rounded product (hipcc would contract r - hi into fma(o, inv, -hi)):
      // the operand is then bitwise x3_cat of the fp32 output
      asm volatile("" : "+v"(r));
      uint32_t h0, l0, h1, l1;
      split_pk(r[0], r[1], h0, l0);
      split_pk(r[2], r[3], h1, l1);
      *reinterpret_cast<uint2*>(op + dt * 16) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(op + H + dt * 16) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(op + 2 * H + dt * 16) = make_uint2(l0, l1);
    }
    return;
  }
  float* const op = out + (TC_ATTN_X3_TOK0 + q) * H + h * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<f32x4*>(op + dt * 16) = o[dt] * inv;
