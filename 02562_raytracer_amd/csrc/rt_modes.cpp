// rt_modes.cpp -- the mode table: what an rt_mode is, stated once (include/rt.h
// rt_mode_desc).  The C ABI layer reads it through mode_desc() (rt_ctx.h), the hosts
// through rt_mode_describe; _ffi.MODE_TABLE is its static mirror (tests/test_modes.py).
// Plain host C++.  A kernel instantiation that is no mode (rt_internal.h
// MODE_W9E1_TRANSPARENT) has no row.
#include "../../include/rt.h"

namespace {

constexpr uint32_t PROG = RT_MODEF_PROGRESSIVE, TEX0 = RT_MODEF_TEXTURE0, LINEAR = RT_MODEF_LINEAR_DISPLAY,
                   AREA = RT_MODEF_AREA_LIGHTS;

// one row per rt_mode, in enum order
constexpr rt_mode_desc kModes[] = {
    {RT_MODE_W1E6, RT_FAMILY_WORKSHEET1, 0, 0, "W1E6", "w1e6.wgsl"},
    {RT_MODE_W6E1, RT_FAMILY_PRIMARY, 0, 0, "W6E1", "w6e1.wgsl"},
    {RT_MODE_PROJECT, RT_FAMILY_PRIMARY, 0, 0, "PROJECT", "project.wgsl"},
    {RT_MODE_W7E3, RT_FAMILY_PATH, PROG | AREA, 0, "W7E3", "w7e3.wgsl"},
    {RT_MODE_W9E1, RT_FAMILY_PATH, PROG, 0, "W9E1", "w9e1.wgsl"},
    {RT_MODE_W8E1, RT_FAMILY_PATH, PROG | AREA, 0, "W8E1", "w8e1.wgsl"},
    {RT_MODE_W8E2, RT_FAMILY_PATH, PROG | AREA, 0, "W8E2", "w8e2.wgsl"},
    {RT_MODE_W8E3, RT_FAMILY_PATH, PROG | AREA, 0, "W8E3", "w8e3.wgsl"},
    {RT_MODE_W9E2, RT_FAMILY_PATH, PROG, 0, "W9E2", "w9e2.wgsl"},
    {RT_MODE_W6E2, RT_FAMILY_DIRECT, 0, 0, "W6E2", "w6e2.wgsl"},
    {RT_MODE_W7E1, RT_FAMILY_DIRECT, PROG, 0, "W7E1", "w7e1.wgsl"},
    {RT_MODE_W7E2, RT_FAMILY_DIRECT, PROG, 0, "W7E2", "w7e2.wgsl"},
    {RT_MODE_W6E3, RT_FAMILY_DIRECT, 0, 0, "W6E3", "w6e3.wgsl"},
    {RT_MODE_W9E3, RT_FAMILY_PATH, PROG, 0, "W9E3", "w9e3.wgsl"},
    {RT_MODE_W5E2, RT_FAMILY_SWEEP, 0, 0, "W5E2", "w5e2.wgsl"},
    {RT_MODE_W5E3, RT_FAMILY_SWEEP, 0, 0, "W5E3", "w5e3.wgsl"},
    {RT_MODE_W5E4, RT_FAMILY_SWEEP, 0, 0, "W5E4", "w5e4.wgsl"},
    {RT_MODE_W5E5, RT_FAMILY_SWEEP, 0, 0, "W5E5", "w5e5.wgsl"},
    {RT_MODE_W2E1, RT_FAMILY_ANALYTIC, 0, 0, "W2E1", "w2e1.wgsl"},
    {RT_MODE_W2E2, RT_FAMILY_ANALYTIC, 0, 0, "W2E2", "w2e2.wgsl"},
    {RT_MODE_W2E3, RT_FAMILY_ANALYTIC, 0, 0, "W2E3", "w2e3.wgsl"},
    {RT_MODE_W2E4, RT_FAMILY_ANALYTIC, 0, 0, "W2E4", "w2e4.wgsl"},
    {RT_MODE_W2E5, RT_FAMILY_ANALYTIC, 0, 0, "W2E5", "w2e5.wgsl"},
    {RT_MODE_W3E1, RT_FAMILY_ANALYTIC, TEX0, 0, "W3E1", "w3e1.wgsl"},
    {RT_MODE_W3E2, RT_FAMILY_ANALYTIC, TEX0, 0, "W3E2", "w3e2.wgsl"},
    {RT_MODE_W3E3, RT_FAMILY_ANALYTIC, TEX0, 0, "W3E3", "w3e3.wgsl"},
    {RT_MODE_W3E4, RT_FAMILY_ANALYTIC, TEX0, 0, "W3E4", "w3e4.wgsl"},
    {RT_MODE_W1E2, RT_FAMILY_WORKSHEET1, LINEAR, 0, "W1E2", "w1e2.wgsl"},
    {RT_MODE_W1E3, RT_FAMILY_WORKSHEET1, LINEAR, 0, "W1E3", "w1e3.wgsl"},
    {RT_MODE_W1E4, RT_FAMILY_WORKSHEET1, 0, 0, "W1E4", "w1e4.wgsl"},
    {RT_MODE_W1E5, RT_FAMILY_WORKSHEET1, 0, 0, "W1E5", "w1e5.wgsl"},
};
constexpr int kCount = (int)(sizeof kModes / sizeof kModes[0]);
static_assert(kCount == RT_MODE_COUNT, "one row per rt_mode");

constexpr bool rows_in_enum_order()
{
    for (int i = 0; i < kCount; i++)
        if (kModes[i].mode != i) return false;
    return true;
}
static_assert(rows_in_enum_order(), "row i describes mode i");

}  // namespace

// the row of `mode`, null for a value that is no rt_mode (rt_ctx.h)
const rt_mode_desc* mode_desc(rt_mode mode)
{
    const int m = (int)mode;
    return m >= 0 && m < kCount ? &kModes[m] : nullptr;
}

extern "C" int rt_mode_describe(int mode, rt_mode_desc* out)
{
    const rt_mode_desc* d = mode_desc((rt_mode)mode);
    if (!d || !out) return RT_E_INVALID;
    *out = *d;
    return RT_OK;
}

// the analytic objects a path mode's shader tests beside the mesh and that leave no primary id
// (rt.h "denoise / Guide with objects"); W6E3 renders the balls too but is no path mode
extern "C" int rt_guide_objects(int mode, uint32_t* objects)
{
    if (!mode_desc((rt_mode)mode) || !objects) return RT_E_INVALID;
    *objects = mode == RT_MODE_W8E1 || mode == RT_MODE_W8E2 || mode == RT_MODE_W8E3 ? RT_GUIDE_BALLS
               : mode == RT_MODE_W9E2 || mode == RT_MODE_W9E3                      ? RT_GUIDE_PLANE
                                                                                   : 0u;
    return RT_OK;
}
