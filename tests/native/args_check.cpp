// args_check.cpp -- the buffer checks of the post-process entry points (csrc/rt_args.h), on
// the host alone: null, alignment and aliasing over one table, in that order, with addresses
// that are never dereferenced.  Includes rt_args.h only.  Exit status 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "rt_args.h"

namespace {

int bad = 0;
void expect(bool ok, const char* what)
{
    if (ok) return;
    std::printf("MISMATCH %s\n", what);
    bad++;
}

const void* at(uintptr_t a) { return reinterpret_cast<const void*>(a); }
bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

BufRange in(uintptr_t a, uint64_t bytes, uint32_t align = 4, const char* name = "in") { return {at(a), bytes, align, false, false, name}; }
BufRange out(uintptr_t a, uint64_t bytes, uint32_t align = 4, const char* name = "out") { return {at(a), bytes, align, true, false, name}; }
BufRange opt(BufRange r)
{
    r.optional = true;
    return r;
}

void null_buffers()
{
    // an optional null is skipped by the null, the alignment and the overlap test (its
    // range [0, 64) would overlap the output at 32)
    const BufRange a[] = {in(0x1000, 64), opt(in(0, 64, 16, "count")), out(32, 16)};
    expect(buffers_fault(a).empty(), "an optional null input is skipped");
    const BufRange b[] = {in(0x1000, 64), opt(out(0, 1 << 20, 16, "out_var"))};
    expect(buffers_fault(b).empty(), "an optional null output is skipped");
    const BufRange c[] = {in(0x1000, 64), in(0, 64, 4, "ids"), out(0x2000, 64)};
    expect(has(buffers_fault(c), "null buffer") && has(buffers_fault(c), "ids"), "a required null input is refused by name");
    const BufRange d[] = {in(0x1000, 64), out(0, 64, 4, "var")};
    expect(has(buffers_fault(d), "null buffer") && has(buffers_fault(d), "var"), "a required null output is refused by name");
    const BufRange e[] = {opt(in(0x1001, 64, 4, "count"))};
    expect(has(buffers_fault(e), "count must be 4-byte aligned"), "an optional buffer that is given is checked");
}

void alignment()
{
    for (uint32_t al : {16u, 8u, 4u}) {
        const BufRange off[] = {in(0x1000 + al / 2, 64, al, "buf")};
        const std::string why = buffers_fault(off);
        expect(has(why, "buf must be") && has(why, (std::to_string(al) + "-byte aligned").c_str()), "+align/2 is refused");
        const BufRange on[] = {in(0x1000 + al, 64, al, "buf")};
        expect(buffers_fault(on).empty(), "+align is accepted");
        const BufRange oo[] = {in(0x1000, 64, 16), out(0x2000 + al / 2, 64, al, "dst")};
        expect(has(buffers_fault(oo), "dst must be"), "an output at +align/2 is refused");
    }
}

void aliasing()
{
    const BufRange a[] = {in(0x1000, 64), in(0x1020, 64), in(0x1000, 64), out(0x2000, 64)};
    expect(buffers_fault(a).empty(), "two inputs may overlap, and be equal");
    const BufRange b[] = {in(0x1000, 64, 4, "color"), out(0x103F, 64, 1, "dst")};
    expect(has(buffers_fault(b), "the output dst overlaps color"), "an output that starts on an input's last byte");
    const BufRange c[] = {out(0x1000, 65, 1, "dst"), in(0x1040, 64, 4, "color")};
    expect(has(buffers_fault(c), "the output dst overlaps color"), "an output whose last byte is an input's first");
    const BufRange d[] = {in(0x1000, 64), out(0x1040, 64), in(0x1080, 64)};
    expect(buffers_fault(d).empty(), "adjacent ranges are accepted");
    const BufRange e[] = {in(0x1000, 16), out(0x2000, 64, 4, "nz"), out(0x2020, 64, 4, "dz")};
    expect(has(buffers_fault(e), "the output nz overlaps dz"), "two outputs overlapping are refused");
    const BufRange f[] = {out(0x2020, 64, 4, "dz"), in(0x1000, 16), out(0x2000, 64, 4, "nz")};
    expect(has(buffers_fault(f), "the output dz overlaps nz"), "two outputs overlapping, either order");
    const BufRange g[] = {in(0x3000, 256, 16, "accum"), out(0x3000, 256, 16, "out")};
    expect(has(buffers_fault(g), "the output out overlaps accum"), "an output equal to an input is refused");
    const BufRange h[] = {in(0x3000, 256), out(0x3010, 16)};
    expect(!buffers_fault(h).empty(), "an output inside an input is refused");
    const BufRange i[] = {in(0x3010, 16), out(0x3000, 256)};
    expect(!buffers_fault(i).empty(), "an input inside an output is refused");
    expect(placement_fault(g).empty(), "placement_fault alone does not look at aliasing");
}

void top_of_the_address_space()
{
    // a + bytes wraps to 0 for a range that ends at UINTPTR_MAX + 1: a test by the sums
    // would call the first pair disjoint and could call the second overlapping
    const uintptr_t top = UINTPTR_MAX - 63;   // [top, top + 64) ends with the last byte
    expect(ranges_overlap(top, 64, top + 32, 32), "a range inside one that ends at the top overlaps it");
    expect(ranges_overlap(top + 32, 32, top, 64), "... in either order");
    expect(!ranges_overlap(top, 64, 0x1000, 64), "a low range does not overlap one that ends at the top");
    expect(!ranges_overlap(0x1000, 64, top, 64), "... in either order");
    expect(!ranges_overlap(top - 64, 64, top, 64), "adjacent below the top range");
    const BufRange a[] = {in(top, 64, 1, "hist"), out(top + 63, 1, 1, "dst")};
    expect(has(buffers_fault(a), "the output dst overlaps hist"), "the last byte of the address space is an overlap");
    const BufRange b[] = {in(0x1000, 64), out(top, 64, 1)};
    expect(buffers_fault(b).empty(), "an output that ends at the top and a low input are accepted");
    expect(!ranges_overlap(0x1000, 0, 0x1000, 64) && !ranges_overlap(0x1000, 64, 0x1010, 0), "an empty range overlaps nothing");
}

void first_failing_class_wins()
{
    // null (the last row) before alignment (the first) before aliasing (the middle two)
    const BufRange a[] = {in(0x1002, 64, 4, "mis"), in(0x2000, 64, 4, "src"), out(0x2000, 64, 4, "dst"), in(0, 64, 4, "gone")};
    expect(has(buffers_fault(a), "null buffer") && has(buffers_fault(a), "gone"), "null wins over alignment and aliasing");
    const BufRange b[] = {in(0x2000, 64, 4, "src"), out(0x2000, 64, 4, "dst"), in(0x1002, 64, 4, "mis")};
    expect(has(buffers_fault(b), "mis must be 4-byte aligned"), "alignment wins over aliasing");
    const BufRange c[] = {in(0x2000, 64, 4, "src"), out(0x2000, 64, 4, "dst")};
    expect(has(buffers_fault(c), "overlaps"), "aliasing is found when the rest holds");
}

void value_checks()
{
    uint64_t npix = 1;
    expect(frame_fault(0, 77, &npix).empty() && npix == 0, "an empty frame is a frame");
    expect(frame_fault(46341, 46341, &npix) == "the frame is too large" && npix == 46341ull * 46341ull, "2^31 pixels and more");
    expect(frame_fault(32768, 65535, &npix).empty(), "just under 2^31 pixels");
    const uint32_t res[2] = {640, 480};
    expect(resolution_fault(res, 640, 480).empty() && !resolution_fault(res, 480, 640).empty(), "the uniforms' resolution");
    expect(filter_fault(1, 4.0f, 1.0f).empty() && filter_fault(5, 4.0f, 1.0f).empty(), "levels 1 and 5");
    expect(!filter_fault(0, 4.0f, 1.0f).empty() && !filter_fault(6, 4.0f, 1.0f).empty(), "levels 0 and 6");
    expect(!filter_fault(3, 0.0f, 1.0f).empty() && !filter_fault(3, 4.0f, NAN).empty(), "a sigma that is zero or NaN");
    expect(noise_fault(2, 1e-3f).empty() && !noise_fault(1, 1e-3f).empty() && !noise_fault(2, 0.0f).empty(), "n and floor");
    expect(adaptive_fault(0.0f, 1e-3f, 2, RT_ADAPT_TILE).empty() && !adaptive_fault(0.05f, 1e-3f, 1, RT_ADAPT_TILE).empty() &&
               !adaptive_fault(NAN, 1e-3f, 16, RT_ADAPT_PIXEL).empty() && !adaptive_fault(0.05f, 1e-3f, 16, 2).empty(),
           "the adaptive rule's parameters");
}

}  // namespace

int main()
{
    null_buffers();
    alignment();
    aliasing();
    top_of_the_address_space();
    first_failing_class_wins();
    value_checks();
    std::printf("args_check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
