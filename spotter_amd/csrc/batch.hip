// Cross-process batching (spotter_amd/shared_batch.py): host-memory registration and the segment copy that
// gathers the waiting replicas' images into one batch and scatters its rows back, one launch each.
#include <climits>
#include <cstdint>
#include <map>
#include <mutex>

#include "common.h"

namespace sp {
namespace {

constexpr int kCopyThreads = 256;
constexpr int kCopyVecPerThread = SP_COPY_BLOCK_ELEMS / 4 / kCopyThreads;  // 16-byte vectors a thread moves
static_assert(kCopyVecPerThread * 4 * kCopyThreads == SP_COPY_BLOCK_ELEMS, "block elems = threads x vectors x 4");

// The kernel's by-value argument: the caller's segments as 32-bit words, and first_block[s] = the first workgroup
// of segment s (first_block[n] = the grid). An empty segment shares its successor's first workgroup.
struct CopyTable {
  const uint32_t* src[SP_COPY_MAX_SEGMENTS];
  uint32_t* dst[SP_COPY_MAX_SEGMENTS];
  long long elems[SP_COPY_MAX_SEGMENTS];
  int first_block[SP_COPY_MAX_SEGMENTS + 1];
  int n;
};

__global__ __launch_bounds__(kCopyThreads) void copy_segments_kernel(const CopyTable t) {
  const int b = blockIdx.x, tid = threadIdx.x;
  // the last segment whose first workgroup is <= b: never an empty one (its successor starts at the same b)
  int s = 0, hi = t.n;
  while (hi - s > 1) {
    const int mid = (s + hi) >> 1;
    if (t.first_block[mid] <= b) s = mid; else hi = mid;
  }
  const uint32_t* __restrict__ src = t.src[s];
  uint32_t* __restrict__ dst = t.dst[s];
  const long long elems = t.elems[s];
  const long long start = (long long)(b - t.first_block[s]) * SP_COPY_BLOCK_ELEMS;
  const long long end = start + SP_COPY_BLOCK_ELEMS < elems ? start + SP_COPY_BLOCK_ELEMS : elems;
  // [vs, ve): the 16-byte vectors of this block. start is a multiple of 4 elements, so with src and dst at the
  // same offset from 16-byte alignment every block's first aligned element is start + head.
  const unsigned sa = (unsigned)((uintptr_t)src & 15u), da = (unsigned)((uintptr_t)dst & 15u);
  long long vs = end, ve = end;
  if (sa == da) {
    const long long head = ((16u - da) & 15u) >> 2;
    if (start + head < end) {
      vs = start + head;
      ve = vs + ((end - vs) & ~3LL);
    }
  }
  const int nvec = (int)((ve - vs) >> 2);  // <= SP_COPY_BLOCK_ELEMS / 4
  if (nvec > 0) {
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src + vs);
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + vs);
    uint4 r[kCopyVecPerThread];
#pragma unroll
    for (int k = 0; k < kCopyVecPerThread; ++k) {
      const int v = tid + k * kCopyThreads;
      if (v < nvec) {
        SP_BCHECK(vs + 4LL * v + 3, elems);
        r[k] = s4[v];
      }
    }
#pragma unroll
    for (int k = 0; k < kCopyVecPerThread; ++k) {
      const int v = tid + k * kCopyThreads;
      if (v < nvec) d4[v] = r[k];
    }
  }
  for (long long e = start + tid; e < vs; e += kCopyThreads) {  // head (or the whole block when unaligned)
    SP_BCHECK(e, elems);
    dst[e] = src[e];
  }
  for (long long e = ve + tid; e < end; e += kCopyThreads) {  // tail
    SP_BCHECK(e, elems);
    dst[e] = src[e];
  }
}

constexpr uintptr_t kPage = 4096;
std::mutex g_reg_mutex;
std::map<uintptr_t, int64_t>& registered() {  // base -> bytes of every range sp_host_register pinned
  static std::map<uintptr_t, int64_t> m;
  return m;
}

}  // namespace
}  // namespace sp

extern "C" int sp_copy_segments(const sp_copy_segments_desc* d, void* stream) {
  SP_ARG_CHECK(d != nullptr, "sp_copy_segments: null descriptor");
  SP_ARG_CHECK(d->n >= 1 && d->n <= SP_COPY_MAX_SEGMENTS, "sp_copy_segments: n %d outside [1, %d]", d->n,
               SP_COPY_MAX_SEGMENTS);
  sp::CopyTable t;
  memset(&t, 0, sizeof(t));
  long long blocks = 0;
  for (int s = 0; s < d->n; ++s) {
    const sp_copy_segment& g = d->seg[s];
    SP_ARG_CHECK(g.elems >= 0, "sp_copy_segments: segment %d has elems %lld < 0", s, (long long)g.elems);
    if (g.elems > 0) {
      SP_ARG_CHECK(g.src != nullptr && g.dst != nullptr, "sp_copy_segments: segment %d has a null pointer", s);
      SP_ARG_CHECK(((uintptr_t)g.src & 3u) == 0 && ((uintptr_t)g.dst & 3u) == 0,
                   "sp_copy_segments: segment %d has a pointer that is not 4-byte aligned", s);
    }
    t.src[s] = reinterpret_cast<const uint32_t*>(g.src);
    t.dst[s] = reinterpret_cast<uint32_t*>(g.dst);
    t.elems[s] = g.elems;
    t.first_block[s] = (int)blocks;
    blocks += (g.elems + SP_COPY_BLOCK_ELEMS - 1) / SP_COPY_BLOCK_ELEMS;
    SP_ARG_CHECK(blocks <= INT_MAX, "sp_copy_segments: more than 2^31 - 1 workgroups at segment %d", s);
  }
  t.n = d->n;
  t.first_block[d->n] = (int)blocks;
  if (blocks == 0) return 0;  // every segment empty
  hipLaunchKernelGGL(sp::copy_segments_kernel, dim3((unsigned)blocks), dim3(sp::kCopyThreads), 0,
                     sp::as_stream(stream), t);
  return sp::check_launch("sp_copy_segments");
}

extern "C" int sp_host_register(void* p, int64_t bytes, void** dev_ptr) {
  SP_ARG_CHECK(p != nullptr, "sp_host_register: null pointer");
  SP_ARG_CHECK(dev_ptr != nullptr, "sp_host_register: null dev_ptr");
  SP_ARG_CHECK(bytes > 0, "sp_host_register: bytes %lld <= 0", (long long)bytes);
  const uintptr_t a = (uintptr_t)p;
  SP_ARG_CHECK((a & (sp::kPage - 1)) == 0, "sp_host_register: pointer %p is not aligned to %d bytes", p,
               (int)sp::kPage);
  std::lock_guard<std::mutex> lk(sp::g_reg_mutex);
  auto& reg = sp::registered();
  for (const auto& r : reg)
    SP_ARG_CHECK(a + (uintptr_t)bytes <= r.first || r.first + (uintptr_t)r.second <= a,
                 "sp_host_register: %p + %lld overlaps the registered range %p + %lld", p, (long long)bytes,
                 (void*)r.first, (long long)r.second);
  hipError_t e = hipHostRegister(p, (size_t)bytes, hipHostRegisterMapped);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    sp::set_error("sp_host_register: hipHostRegister(%p, %lld): %s", p, (long long)bytes, hipGetErrorString(e));
    return (int)e;
  }
  void* dp = nullptr;
  e = hipHostGetDevicePointer(&dp, p, 0);
  if (e != hipSuccess || dp == nullptr) {
    (void)hipGetLastError();
    (void)hipHostUnregister(p);
    sp::set_error("sp_host_register: hipHostGetDevicePointer(%p): %s", p, hipGetErrorString(e));
    return e != hipSuccess ? (int)e : -2;
  }
  reg[a] = bytes;
  *dev_ptr = dp;
  return 0;
}

extern "C" int sp_host_unregister(void* p) {
  SP_ARG_CHECK(p != nullptr, "sp_host_unregister: null pointer");
  std::lock_guard<std::mutex> lk(sp::g_reg_mutex);
  auto& reg = sp::registered();
  auto it = reg.find((uintptr_t)p);
  SP_ARG_CHECK(it != reg.end(), "sp_host_unregister: %p is not registered", p);
  hipError_t e = hipHostUnregister(p);
  reg.erase(it);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    sp::set_error("sp_host_unregister: hipHostUnregister(%p): %s", p, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}
