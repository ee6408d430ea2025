// rt_args.h -- the argument checks the post-process entry points of the C ABI share
// (rt_estimate.cpp, rt_denoise_api.cpp, rt_temporal_api.cpp): one table of buffers per entry
// point, checked for null, alignment and aliasing in that order, and the value checks several
// of them make.  Every check returns the reason it refuses, without the entry point's name, or
// an empty string; refuse() (rt_ctx.h) turns a reason into RT_E_INVALID and the context's
// message.  Host code with no HIP in it: tests/native/args_check.cpp compiles it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/rt.h"

// One caller-owned buffer of an entry point: `bytes` at p, which must be a multiple of
// `align`; out: the entry point writes it; optional: it may be null (and is then skipped).
struct BufRange {
    const void* p;
    uint64_t bytes;
    uint32_t align;
    bool out, optional;
    const char* name;
};

// do [a, a + an) and [b, b + bn) share a byte?  By the distance of the two starts, which
// cannot wrap as a + an can for a range that ends at the top of the address space
inline bool ranges_overlap(uintptr_t a, uint64_t an, uintptr_t b, uint64_t bn)
{
    if (!an || !bn) return false;
    return a <= b ? b - a < an : a - b < bn;
}

// a required buffer that is null, else a buffer that is not aligned
inline std::string placement_fault(const BufRange* r, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!r[i].p && !r[i].optional) return std::string("null buffer: ") + r[i].name;
    for (size_t i = 0; i < n; i++)
        if (r[i].p && (uintptr_t)r[i].p % r[i].align)
            return std::string(r[i].name) + " must be " + std::to_string(r[i].align) + "-byte aligned";
    return std::string();
}
// an output that overlaps an input or another output (inputs may overlap one another)
inline std::string alias_fault(const BufRange* r, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        if (!r[i].out || !r[i].p) continue;
        for (size_t j = 0; j < n; j++) {
            if (j == i || !r[j].p || (r[j].out && j < i)) continue;   // (two outputs: compared once)
            if (ranges_overlap((uintptr_t)r[i].p, r[i].bytes, (uintptr_t)r[j].p, r[j].bytes))
                return std::string("the output ") + r[i].name + " overlaps " + r[j].name;
        }
    }
    return std::string();
}
// the first failing class wins: null, then alignment, then aliasing
inline std::string buffers_fault(const BufRange* r, size_t n)
{
    std::string why = placement_fault(r, n);
    return why.empty() ? alias_fault(r, n) : why;
}
template <size_t N>
std::string placement_fault(const BufRange (&r)[N])
{
    return placement_fault(r, N);
}
template <size_t N>
std::string buffers_fault(const BufRange (&r)[N])
{
    return buffers_fault(r, N);
}

// ---- value checks ----
// *npix = width x height, which the kernels index with 32 bits
inline std::string frame_fault(uint32_t width, uint32_t height, uint64_t* npix)
{
    *npix = (uint64_t)width * height;
    return *npix >= (1ull << 31) ? "the frame is too large" : "";
}
// the frame the context's uniforms were set for
inline std::string resolution_fault(const uint32_t resolution[2], uint32_t width, uint32_t height)
{
    return resolution[0] != width || resolution[1] != height ? "the uniforms' resolution is not width x height" : "";
}
// a mask of the analytic objects a guide knows (rt.h RT_GUIDE_*)
inline std::string guide_objects_fault(uint32_t objects)
{
    return objects & ~(RT_GUIDE_BALLS | RT_GUIDE_PLANE) ? "objects has a bit outside RT_GUIDE_BALLS | RT_GUIDE_PLANE" : "";
}
inline std::string filter_fault(uint32_t levels, float sigma_l, float sigma_z)
{
    if (levels < 1 || levels > 5) return "levels must be in 1..5";
    if (!(sigma_l > 0.0f) || !(sigma_z > 0.0f)) return "the sigmas must be > 0";
    return "";
}
inline std::string noise_fault(uint32_t n, float floor)
{
    if (n < 2) return "the standard error needs n >= 2 iterations";
    if (!(floor > 0.0f)) return "floor must be > 0";
    return "";
}
inline std::string adaptive_fault(float target, float floor, uint32_t min_samples, int vote)
{
    if (min_samples < 2) return "min_samples must be >= 2";
    if (!(target >= 0.0f)) return "target must be >= 0 and not NaN";
    if (!(floor > 0.0f)) return "floor must be > 0";
    if (vote != RT_ADAPT_PIXEL && vote != RT_ADAPT_TILE) return "vote must be RT_ADAPT_PIXEL or RT_ADAPT_TILE";
    return "";
}
