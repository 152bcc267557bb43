// K24 jpeg_huffman_wide — K23's Huffman stage (jpeg_huff.hip) for scans K23
// cannot take and for the reduced-size decode: a scan of up to 32 MiB of
// unstuffed data (262,144 subsequences of 128 bytes against K23's 2048), decoded
// by many workgroups per image, into the compact coefficient buffer of any
// jpeg_scale (1, 2, 4, 8), byte for byte the buffer of the host entropy decoder
// at that scale.  The stream buffer is what tcamd_host_jpeg_stream_pack_wide
// writes (csrc/host/jpeg.cc).
//
// An image's subsequences are dealt in order into chunks of chunk_subs (1024
// by default, one per thread); the grid of every launch is the flattened list of
// all chunks of up to 64 images, one workgroup of 1024 threads per chunk.  The
// per-subsequence state (exit, last entry, three DC sums, block count, segment:
// 28 bytes) and 72 bytes per chunk live in a device workspace of the caller;
// LDS holds the Huffman tables (6 x 1416 bytes) or the 32 KiB of the scan.
//
// Workgroups never wait for each other inside a launch: there is no flag, no
// counter, no spin loop and no cooperative launch.  What chunk k hands to chunk
// k + 1 crosses a kernel boundary, so a call is a sequence of launches on the
// caller's stream, none of which depends on anything read back:
//   status words zeroed, init, sync 0, sync 1 .. R, count, carry, write
// with R = the largest chunk count of an image of the call - 1 (a sync launch
// in which a chunk's entry did not change returns at once for that chunk).
// The phases, the workspace and every bound are in kernels/jpeg_huff_wide_core.h,
// which the host library compiles too: its emulation runs the same sequence
// launch by launch, workgroup by workgroup, thread by thread.
//
// Every workgroup of every launch validates the header again; errors end in
// status[image] by atomicMax.  The kernels never trap and write only inside
// [coef, coef + coef_bytes), the status words and the workspace.

#include "kernels/common.h"
#include "kernels/jpeg_huff_wide_core.h"

using namespace tcamd;
using namespace tcamd_jhuff;

namespace {

struct WideParams {
  const uint8_t* stream[kWideMaxImgs];
  uint8_t* coef[kWideMaxImgs];
  uint32_t nsub[kWideMaxImgs];             // from the pack; the header must agree
  uint32_t sub_base[kWideMaxImgs];         // the image's first subsequence in the workspace
  uint32_t chunk_base[kWideMaxImgs + 1];   // the image's first chunk in the grid and the workspace
  uint32_t n_imgs, cs;
  uint8_t* ws;
  uint32_t* status;
};

struct Ctx {
  WideGeo wg;
  WideWs w;
  Chunk c;
  uint8_t* coef;
  uint32_t* status;
};

// Uniform over the workgroup: image m, its chunk k.  False when the header does not hold or
// differs from what the host sized the grid and the workspace by.
__device__ __forceinline__ bool enter(const WideParams& p, uint32_t m, uint32_t k, Ctx& x) {
  x.status = p.status + m;
  x.coef = p.coef[m];
  if (!read_header_wide(p.stream[m], x.wg) || x.wg.g.nsub != p.nsub[m]) return false;
  x.c = chunk_of(x.wg.g, p.cs, k);
  const uint32_t total_chunks = p.chunk_base[p.n_imgs], last = p.n_imgs - 1;
  const WideWs all = wide_ws_carve(p.ws, (uint64_t)p.sub_base[last] + p.nsub[last], total_chunks);
  x.w = wide_ws_of_image(all, p.sub_base[m], p.chunk_base[m]);
  return true;
}

// the image of workgroup `block` of a grid over all chunks: the last whose first chunk is at or before it
__device__ __forceinline__ uint32_t image_of(const WideParams& p, uint32_t block) {
  uint32_t lo = 0, hi = p.n_imgs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (p.chunk_base[mid] <= block) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads) jpeg_huffman_wide_init(WideParams p) {
  const uint32_t m = image_of(p, blockIdx.x);
  Ctx x;
  if (!enter(p, m, blockIdx.x - p.chunk_base[m], x)) {
    if (threadIdx.x == 0) status_max(x.status, kBadHeader);
    return;
  }
  wide_init(threadIdx.x, x.wg, x.w, x.c, x.coef, x.status);
}

// launch r of the sync sequence
__global__ void __launch_bounds__(kThreads) jpeg_huffman_wide_sync(WideParams p, uint32_t r) {
  __shared__ HuffTab tabs[kMaxTabs];
  __shared__ uint32_t go;
  const uint32_t tid = threadIdx.x, m = image_of(p, blockIdx.x);
  Ctx x;
  if (!enter(p, m, blockIdx.x - p.chunk_base[m], x)) return;
  if (tid == 0) {
    go = *x.status == kOk;  // the segment table held
    if (go && r != 0 && !wide_take(x.w, x.c, r)) {
      wide_publish(x.w, x.c, r);  // nothing new: what it published before stands
      go = 0;
    }
  }
  __syncthreads();
  if (!go) return;
  wide_load_tables(tid, x.wg.g, tabs);
  __syncthreads();
  for (uint32_t round = 0; round <= x.c.n; ++round) {
    if (round) {
      wide_sync_read(tid, x.w, x.c);
      __syncthreads();
    }
    const bool any = wide_sync_decode(tid, x.wg.g, tabs, x.w, x.c);
    if (!__syncthreads_or(any)) break;
  }
  if (tid == 0) wide_publish(x.w, x.c, r);
}

// The inclusive segmented scan of lds[kThreads] (jpeg_huff_wide_core.h scan_step).
__device__ __forceinline__ void scan(uint32_t tid, uint32_t n, Acc* lds) {
  for (uint32_t d = 1; d < n; d <<= 1) {
    const Acc v = scan_step(tid, d, lds);
    __syncthreads();
    lds[tid] = v;
    __syncthreads();
  }
}

__device__ __forceinline__ bool status_ok(const Ctx& x, uint32_t* flag) {
  if (threadIdx.x == 0) *flag = *x.status == kOk;
  __syncthreads();
  return *flag != 0;
}

__global__ void __launch_bounds__(kThreads) jpeg_huffman_wide_count(WideParams p) {
  __shared__ Acc lds[kThreads];
  __shared__ uint32_t go;
  const uint32_t tid = threadIdx.x, m = image_of(p, blockIdx.x);
  Ctx x;
  if (!enter(p, m, blockIdx.x - p.chunk_base[m], x)) return;
  if (!status_ok(x, &go)) return;
  lds[tid] = wide_count_load(tid, x.w, x.c);
  __syncthreads();
  scan(tid, x.c.n, lds);
  wide_count_store(tid, x.w, x.c, lds);
}

// one workgroup per image: the scan over its chunks' totals, kThreads chunks at a time
__global__ void __launch_bounds__(kThreads) jpeg_huffman_wide_carry(WideParams p) {
  __shared__ Acc lds[kThreads];
  __shared__ uint32_t go;
  const uint32_t tid = threadIdx.x;
  Ctx x;
  if (!enter(p, blockIdx.x, 0, x)) return;
  if (!status_ok(x, &go)) return;
  Acc carry{0, 0, 0, 0, 0};
  for (uint32_t base = 0; base < x.c.nchunk; base += kThreads) {
    lds[tid] = wide_tile_load(tid, x.w, base, x.c.nchunk);
    __syncthreads();
    scan(tid, kThreads, lds);
    wide_tile_store(tid, x.w, base, x.c.nchunk, carry, lds);
    carry = combine(carry, lds[kThreads - 1]);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kThreads) jpeg_huffman_wide_write(WideParams p) {
  __shared__ HuffTab tabs[kMaxTabs];
  __shared__ uint32_t go;
  const uint32_t tid = threadIdx.x, m = image_of(p, blockIdx.x);
  Ctx x;
  if (!enter(p, m, blockIdx.x - p.chunk_base[m], x)) return;
  if (!status_ok(x, &go)) return;
  wide_load_tables(tid, x.wg.g, tabs);
  __syncthreads();
  wide_write(tid, x.wg, tabs, x.w, x.c, x.coef, x.status);
}

}  // namespace

// The workspace of a call over images of `total_subsequences` subsequences in `total_chunks`
// chunks (image i: ceil(nsubs[i] / chunk_subs)), in bytes.
extern "C" uint64_t tcamd_jpeg_huffman_wide_workspace(uint64_t total_subsequences, uint64_t total_chunks) {
  return wide_ws_bytes(total_subsequences, total_chunks);
}

// streams / coefs: host arrays of n_imgs device pointers, 16-byte aligned: image i's stream
// buffer (tcamd_host_jpeg_stream_pack_wide) and its coefficient buffer, coef_bytes of its parse
// at the stream's scale.  nsubs: a host array, image i's subsequences as the pack reported them:
// they size the grid, the workspace and the number of launches, and the kernels check them
// against the header.  status: a device array of n_imgs uint32, image i's word 0 or the reason
// (jpeg_huff_core.h Status) its coefficients are not to be used.  workspace: device memory,
// 16-byte aligned, at least tcamd_jpeg_huffman_wide_workspace() of the whole call; its contents
// mean nothing before or after.  chunk_subs: a power of two up to 1024, 0 for 1024.  Images
// past 64 take a further launch sequence.  A null or misaligned pointer, a workspace too small,
// another chunk_subs or an nsubs[i] of 0 or above 262,144 is hipErrorInvalidValue before any launch.
extern "C" int tcamd_jpeg_huffman_wide(const void* const* streams, void* const* coefs, const uint32_t* nsubs,
                                       void* status, void* workspace, uint64_t workspace_bytes, int n_imgs,
                                       uint32_t chunk_subs, void* stream) {
  if (n_imgs < 0) return hipErrorInvalidValue;
  if (n_imgs == 0) return hipSuccess;
  const uint32_t cs = chunk_subs ? chunk_subs : (uint32_t)kThreads;
  if (!chunk_subs_ok(cs)) return hipErrorInvalidValue;
  if (!streams || !coefs || !nsubs || !status || ((uintptr_t)status) % 4 || !workspace || ((uintptr_t)workspace) % 16)
    return hipErrorInvalidValue;
  uint64_t subs = 0, chunks = 0;
  for (int i = 0; i < n_imgs; ++i) {
    if (!streams[i] || !coefs[i] || ((uintptr_t)streams[i]) % 16 || ((uintptr_t)coefs[i]) % 16)
      return hipErrorInvalidValue;
    if (nsubs[i] == 0 || nsubs[i] > kWideMaxSub) return hipErrorInvalidValue;
    subs += nsubs[i];
    chunks += (nsubs[i] + cs - 1) / cs;
  }
  if (workspace_bytes < wide_ws_bytes(subs, chunks)) return hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  for (int base = 0; base < n_imgs; base += kWideMaxImgs) {
    // the launch sequences of a call follow each other on the stream: each has the workspace to itself
    WideParams p;
    const int cnt = n_imgs - base < kWideMaxImgs ? n_imgs - base : kWideMaxImgs;
    uint32_t nsub = 0, nchunk = 0, most = 0;
    for (int i = 0; i < kWideMaxImgs; ++i) {
      const int j = base + (i < cnt ? i : 0);
      p.stream[i] = static_cast<const uint8_t*>(streams[j]);
      p.coef[i] = static_cast<uint8_t*>(coefs[j]);
      p.nsub[i] = nsubs[j];
      p.sub_base[i] = nsub;
      p.chunk_base[i] = nchunk;
      if (i < cnt) {
        const uint32_t c = (nsubs[j] + cs - 1) / cs;
        nsub += nsubs[j];  // at most 64 * 2^18
        nchunk += c;
        most = c > most ? c : most;
      }
    }
    p.chunk_base[kWideMaxImgs] = nchunk;
    p.chunk_base[cnt] = nchunk;
    p.n_imgs = (uint32_t)cnt;
    p.cs = cs;
    p.ws = static_cast<uint8_t*>(workspace);
    p.status = static_cast<uint32_t*>(status) + base;
    int rc = hipMemsetAsync(p.status, 0, sizeof(uint32_t) * (size_t)cnt, s);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(jpeg_huffman_wide_init, dim3(nchunk), dim3(kThreads), 0, s, p);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    for (uint32_t r = 0; r < most; ++r) {
      hipLaunchKernelGGL(jpeg_huffman_wide_sync, dim3(nchunk), dim3(kThreads), 0, s, p, r);
      if ((rc = hipGetLastError()) != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(jpeg_huffman_wide_count, dim3(nchunk), dim3(kThreads), 0, s, p);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    hipLaunchKernelGGL(jpeg_huffman_wide_carry, dim3((unsigned)cnt), dim3(kThreads), 0, s, p);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
    hipLaunchKernelGGL(jpeg_huffman_wide_write, dim3(nchunk), dim3(kThreads), 0, s, p);
    if ((rc = hipGetLastError()) != hipSuccess) return rc;
  }
  return hipSuccess;
}
