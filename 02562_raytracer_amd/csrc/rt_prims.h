// rt_prims.h -- the device primitives the builders and the list builders share
// (rt_prims.hip): a device-wide exclusive scan, a stable radix sort of (key, value)
// pairs, a stream compaction on top of the scan, and the owner of a build's scratch
// allocations; and the small device helpers more than one file uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rt_detmath.h"

namespace rtk {

// out[0..n] = exclusive prefix sums of in[0..n), out[n] = total: out holds n + 1 words
// (in == out allowed); scratch: scan_scratch_words(n)
int scan_exclusive_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* scratch, hipStream_t s);
size_t scan_scratch_words(uint32_t n);
// Stable LSD radix sort of (key, value) pairs over the low 8*passes key bits;
// ping-pongs between (k0,v0) and (k1,v1); returns which pair holds the result.
// hist: radix_hist_words(n)
int radix_sort_pairs(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t n, uint32_t passes,
                     uint32_t* hist, hipStream_t s, int& result_in_second);
size_t radix_hist_words(uint32_t n);
// Stream compaction: list = the indices i < n with flags[i] != 0 (flags in {0, 1}),
// ascending.  offs: n + 1 words (the flags' scan), scan: scan_scratch_words(n), list: n
// words.  The copy of the number of entries (offs[n]) into *count (host) is enqueued
// last: it is there once the caller has synchronised the stream
int compact_flagged(const uint32_t* flags, uint32_t* offs, uint32_t n, uint32_t* scan, uint32_t* list,
                    uint32_t* count, hipStream_t s);

struct DevScratch {   // device allocations freed at scope exit; e: the first failure
    std::vector<void*> p;
    hipError_t e = hipSuccess;
    ~DevScratch()
    {
        for (void* q : p) (void)hipFree(q);
    }
    template <class T>
    T* alloc(size_t count)
    {
        void* q = nullptr;
        if (e == hipSuccess) e = hipMalloc(&q, std::max<size_t>(16, count * sizeof(T)));
        if (e == hipSuccess) p.push_back(q);
        return reinterpret_cast<T*>(q);
    }
};

// monotone float <-> u32 key in f32::total_cmp order (-0 < +0), for integer atomics and sorts
__device__ __forceinline__ uint32_t ord_key(float f)
{
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord_unkey(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// Bbox::from_triangle (Mesh::bboxes, src/mesh.rs:212-227) of the triangle with vertex indices ix
__device__ __forceinline__ void tri_box(const float4* pos, const uint4 ix, float mn[3], float mx[3])
{
    const float4 a = pos[ix.x], b = pos[ix.y], c = pos[ix.z];
    mn[0] = rt_minf(a.x, rt_minf(b.x, c.x));
    mn[1] = rt_minf(a.y, rt_minf(b.y, c.y));
    mn[2] = rt_minf(a.z, rt_minf(b.z, c.z));
    mx[0] = rt_maxf(a.x, rt_maxf(b.x, c.x));
    mx[1] = rt_maxf(a.y, rt_maxf(b.y, c.y));
    mx[2] = rt_maxf(a.z, rt_maxf(b.z, c.z));
}

// Minimum of mn[0..3) and maximum of mx[0..3) over a block of 256 threads, as a tree over
// halves (exact: the order cannot change a min or a max but for the sign of a zero);
// afterwards red[i][0] holds the minima (i < 3) and the maxima (3 <= i < 6)
__device__ __forceinline__ void block_minmax6(float (*red)[256], const float mn[3], const float mx[3])
{
    for (int i = 0; i < 3; i++) {
        red[i][threadIdx.x] = mn[i];
        red[3 + i][threadIdx.x] = mx[i];
    }
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int i = 0; i < 3; i++) {
                red[i][threadIdx.x] = rt_minf(red[i][threadIdx.x], red[i][threadIdx.x + s]);
                red[3 + i][threadIdx.x] = rt_maxf(red[3 + i][threadIdx.x], red[3 + i][threadIdx.x + s]);
            }
        __syncthreads();
    }
}

// Hillis-Steele inclusive scan of one value per thread over a block of NT threads, in NT
// words of LDS the caller owns: part[t] = v(0) + .. + v(t) afterwards, this thread's returned
template <uint32_t NT, class T>
__device__ __forceinline__ T block_scan_inclusive(T* part, T v)
{
    part[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 1; off < NT; off <<= 1) {
        const T a = threadIdx.x >= off ? part[threadIdx.x - off] : T(0);
        __syncthreads();
        part[threadIdx.x] += a;
        __syncthreads();
    }
    return part[threadIdx.x];
}

}  // namespace rtk
