// rt_prims.hip -- the device primitives of rt_prims.h: the device-wide exclusive scan,
// the stable radix sort of (key, value) pairs and the stream compaction.  The builders
// (rt_build.hip, rt_bsp_build.hip) sort and scan with them; the active list of
// RT_OPT_EMPTY_PIXELS (rt_empty.hip) and the live list of the adaptive sampling
// (rt_adaptive.hip) are compactions.
#include "rt_prims.h"

#include "../../include/rt.h"

namespace rtb {

constexpr int kTile = 2048;          // radix sort keys per block (256 threads x 8)

// ------------------------------------------------------------ radix sort
// Stable LSD radix sort of (code, index) pairs, 8-bit digits.  Per pass:
// per-tile digit histograms (digit-major), one exclusive scan, and a stable
// scatter: each tile ranks its keys in order, 256 at a time, with wave64
// match masks (8 ballots) and a per-digit running count across the 4 waves.
__global__ void __launch_bounds__(256) k_rs_hist(const uint32_t* keys, uint32_t n, uint32_t shift, uint32_t ntiles,
                                                 uint32_t* hist)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)kTile;
    for (uint32_t i = threadIdx.x; i < (uint32_t)kTile; i += 256u) {
        const uint32_t k = base + i;
        if (k < n) atomicAdd(&cnt[(keys[k] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of m words in place, one block of 1024 threads
__global__ void __launch_bounds__(1024) k_rs_scan(uint32_t* a, uint32_t m)
{
    __shared__ uint32_t part[1024];
    const uint32_t per = (m + 1023u) / 1024u;
    const uint32_t lo = threadIdx.x * per, hi = min(m, lo + per);
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += a[i];
    uint32_t run = rtk::block_scan_inclusive<1024>(part, s) - s;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t v = a[i];
        a[i] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(256) k_rs_scatter(const uint32_t* kin, const uint32_t* vin, uint32_t n,
                                                    uint32_t shift, uint32_t ntiles, const uint32_t* offs,
                                                    uint32_t* kout, uint32_t* vout)
{
    __shared__ uint32_t gbase[256], running[256], wcnt[4][256], wbase[4][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    gbase[threadIdx.x] = offs[threadIdx.x * ntiles + blockIdx.x];
    running[threadIdx.x] = 0;
    for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64u - lane));
    for (uint32_t r = 0; r < (uint32_t)kTile / 256u; r++) {
        const uint32_t k = blockIdx.x * (uint32_t)kTile + r * 256u + threadIdx.x;
        const bool valid = k < n;
        const uint32_t key = valid ? kin[k] : 0u, val = valid ? vin[k] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t m = __ballot(((d >> b) & 1u) != 0u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (valid && rank == 0) wcnt[wave][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        {
            const uint32_t dd = threadIdx.x;
            uint32_t s = running[dd];
            for (int w = 0; w < 4; w++) {
                const uint32_t c = wcnt[w][dd];
                wbase[w][dd] = s;
                s += c;
                wcnt[w][dd] = 0;
            }
            running[dd] = s;
        }
        __syncthreads();
        if (valid) {
            const uint32_t pos = gbase[d] + wbase[wave][d] + rank;
            kout[pos] = key;
            vout[pos] = val;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------ device-wide exclusive scan
// out[0..n] = exclusive prefix sums of in[0..n), out[n] = total (in == out allowed).
// Reduce-then-scan: 4096-element blocks (256 threads x 16), one-block scan of
// the block sums, then each block scans its elements with its offset.
constexpr uint32_t kScanBlock = 4096;
__global__ void __launch_bounds__(256) k_scan_reduce(const uint32_t* in, uint32_t n, uint32_t* bsum)
{
    __shared__ uint32_t red[256];
    const uint32_t base = blockIdx.x * kScanBlock;
    uint32_t s = 0;
    for (uint32_t i = threadIdx.x; i < kScanBlock; i += 256u)
        if (base + i < n) s += in[base + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t st = 128; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) k_scan_down(const uint32_t* in, uint32_t n, const uint32_t* bsum,
                                                   uint32_t* out)
{
    __shared__ uint32_t part[256];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * 16u;
    uint32_t v[16], s = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        v[i] = base + i < n ? in[base + i] : 0u;
        s += v[i];
    }
    uint32_t run = bsum[blockIdx.x] + rtk::block_scan_inclusive<256>(part, s) - s;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 255u) out[n] = run;
}

}  // namespace rtb

namespace rtk {

namespace {
// the set flags' indices, ascending (offs: the flags' exclusive scan)
__global__ void __launch_bounds__(256) k_compact_scatter(const uint32_t* flags, const uint32_t* offs, uint32_t n,
                                                         uint32_t* list)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n && flags[s]) list[offs[s]] = s;   // offs[s] < the number of set flags <= n
}
}  // namespace

int scan_exclusive_u32(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* scratch, hipStream_t s)
{
    using namespace rtb;
    const uint32_t nb = n ? (n + kScanBlock - 1) / kScanBlock : 1;
    if (n == 0) {
        (void)hipMemsetAsync(out, 0, 4, s);
        return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
    }
    hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(256), 0, s, in, n, scratch);
    hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, scratch, nb);
    hipLaunchKernelGGL(k_scan_down, dim3(nb), dim3(256), 0, s, in, n, scratch, out);
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}
size_t scan_scratch_words(uint32_t n) { return (size_t)(n + rtb::kScanBlock - 1) / rtb::kScanBlock + 16; }

int radix_sort_pairs(uint32_t* k0, uint32_t* v0, uint32_t* k1, uint32_t* v1, uint32_t n, uint32_t passes,
                     uint32_t* hist, hipStream_t s, int& result_in_second)
{
    using namespace rtb;
    const uint32_t ntiles = (n + kTile - 1) / kTile;
    result_in_second = 0;
    for (uint32_t pass = 0; pass < passes && n; pass++) {
        const uint32_t sh = pass * 8u;
        hipLaunchKernelGGL(k_rs_hist, dim3(ntiles), dim3(256), 0, s, k0, n, sh, ntiles, hist);
        hipLaunchKernelGGL(k_rs_scan, dim3(1), dim3(1024), 0, s, hist, 256u * ntiles);
        hipLaunchKernelGGL(k_rs_scatter, dim3(ntiles), dim3(256), 0, s, k0, v0, n, sh, ntiles, hist, k1, v1);
        std::swap(k0, k1);
        std::swap(v0, v1);
        result_in_second ^= 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : RT_E_DEVICE;
}
size_t radix_hist_words(uint32_t n) { return (size_t)256 * ((n + rtb::kTile - 1) / rtb::kTile) + 16; }

int compact_flagged(const uint32_t* flags, uint32_t* offs, uint32_t n, uint32_t* scan, uint32_t* list,
                    uint32_t* count, hipStream_t s)
{
    if (int r = scan_exclusive_u32(flags, offs, n, scan, s)) return r;
    if (n) hipLaunchKernelGGL(k_compact_scatter, dim3((n + 255u) / 256u), dim3(256), 0, s, flags, offs, n, list);
    if (hipGetLastError() != hipSuccess) return RT_E_DEVICE;
    return hipMemcpyAsync(count, offs + n, 4, hipMemcpyDeviceToHost, s) == hipSuccess ? 0 : RT_E_DEVICE;
}

}  // namespace rtk
