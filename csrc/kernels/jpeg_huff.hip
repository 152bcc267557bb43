// K23 jpeg_huffman — the serial half of a baseline JPEG decode on the device:
// the Huffman stage, from the stream buffer the host packs
// (tcamd_host_jpeg_stream_pack, csrc/host/jpeg.cc: one linear pass over the
// blob, no Huffman work) to the coefficient buffer K22 jpeg_decode reads
// (csrc/host/jpeg.h), byte for byte the buffer of the host entropy decoder.
//
// A Huffman stream has no index, but a decoder started at a wrong bit falls
// into step with the right one after a few symbols.  So every segment (restart
// interval) is cut into subsequences of kSubBits = 1024 bits; each is decoded
// from its first bit as if a block began there, then re-decoded from its
// predecessor's exit for as long as that exit keeps changing.  The first
// subsequence of a segment is right, so after round k the first k + 1 are, and
// a round that decodes nothing is the fixed point: the rounds are bounded by
// the subsequence count, with no heuristic cap.  Exclusive sums of the
// completed blocks and of the DC differences then give every subsequence its
// first block and its predictors, and a last decode from the true entries
// writes the values.  The algorithm, the stream buffer and every bound are in
// kernels/jpeg_huff_core.h, which the host library compiles too: its emulation
// of this kernel runs the same phases thread by thread.
//
// One workgroup of 1024 threads per image (grid x), up to 64 images per launch;
// subsequences and segments are strided over the threads, the phases are
// separated by workgroup barriers and nothing is shared between workgroups.
// LDS per workgroup, independent of the image: the Huffman tables (6 x 1416
// bytes) and 24 bytes per subsequence (exit, entry / first block, three DC sums,
// block count, segment) for kMaxSub = 2048 subsequences: 57,652 bytes with the
// status word (sizeof(Work)), static; the code object reports 57,920 with the
// reduction buffer of __syncthreads_or.  That fixes the longest scan the device
// takes, 2048 subsequences = 256 KiB of unstuffed entropy-coded data; the pack
// enforces it and the kernel checks the header again.  Errors (a header that
// does not hold, invalid data) end in status[image]; the kernel never traps and
// writes only inside [coef, coef + coef_bytes) and status.

#include "kernels/common.h"
#include "kernels/jpeg_huff_core.h"

using namespace tcamd;
using namespace tcamd_jhuff;

static_assert(sizeof(Work) <= 64 * 1024, "the workspace is static LDS");

namespace {

constexpr int kMaxImgs = 64;

struct HuffParams {
  const uint8_t* stream[kMaxImgs];
  uint8_t* coef[kMaxImgs];
};

__global__ void __launch_bounds__(kThreads) jpeg_huffman(HuffParams p, uint32_t* __restrict__ status) {
  __shared__ Work w;
  const uint32_t tid = threadIdx.x;
  const uint8_t* stream = p.stream[blockIdx.x];
  uint8_t* coef = p.coef[blockIdx.x];
  Geo g;
  if (!read_header(stream, g)) {  // uniform over the workgroup
    if (tid == 0) status[blockIdx.x] = kBadHeader;
    return;
  }
  if (tid == 0) w.status = kOk;
  __syncthreads();
  phase_init(tid, g, w, coef);
  __syncthreads();
  if (w.status != kOk) {  // uniform: read after the barrier
    if (tid == 0) status[blockIdx.x] = w.status;
    return;
  }
  for (uint32_t round = 0; round <= g.nsub; ++round) {
    if (round) {
      phase_sync_read(tid, g, w);
      __syncthreads();
    }
    const bool any = phase_sync_decode(tid, g, w);
    if (!__syncthreads_or(any)) break;
  }
  phase_count(tid, g, w);
  __syncthreads();
  phase_write(tid, g, w, coef);
  __syncthreads();
  if (tid == 0) status[blockIdx.x] = w.status;
}

}  // namespace

// streams / coefs: host arrays of n_imgs device pointers, 16-byte aligned:
// image i's stream buffer (tcamd_host_jpeg_stream_pack) and its coefficient
// buffer, coef_bytes of its parse.  status: a device array of n_imgs uint32,
// image i's word 0 or the reason (jpeg_huff_core.h Status) its coefficients are
// not to be used.  Images past 64 take further launches.  A null or misaligned
// pointer is hipErrorInvalidValue before any launch.
extern "C" int tcamd_jpeg_huffman(const void* const* streams, void* const* coefs, void* status, int n_imgs,
                                  void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  if (!streams || !coefs || !status || ((uintptr_t)status) % 4) return hipErrorInvalidValue;
  for (int i = 0; i < n_imgs; ++i)
    if (!streams[i] || !coefs[i] || ((uintptr_t)streams[i]) % 16 || ((uintptr_t)coefs[i]) % 16)
      return hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_imgs; base += kMaxImgs) {
    HuffParams p;
    const int cnt = n_imgs - base < kMaxImgs ? n_imgs - base : kMaxImgs;
    for (int i = 0; i < kMaxImgs; ++i) {
      const int j = base + (i < cnt ? i : 0);
      p.stream[i] = static_cast<const uint8_t*>(streams[j]);
      p.coef[i] = static_cast<uint8_t*>(coefs[j]);
    }
    hipLaunchKernelGGL(jpeg_huffman, dim3((unsigned)cnt), dim3(kThreads), 0, s, p,
                       static_cast<uint32_t*>(status) + base);
    const int rc = hipGetLastError();
    if (rc != hipSuccess) return rc;
  }
  return hipSuccess;
}
