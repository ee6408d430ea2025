// modes_check.cpp -- the mode table (csrc/rt_modes.cpp) against literal expectations, on the
// host alone: rt_mode_describe over and past the enum, and the shader -> row lookup of the
// C++ host layer (raytracer.hpp mode_of_shader) for every scene's shader file, the empty
// string and a 4 KiB string.  Linked with rt_modes.cpp only.  Exit status 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <string>

#include "raytracer.hpp"

namespace {

struct Want {
    const char* name;
    const char* shader;
    int family;
    unsigned flags;
};
const unsigned P = RT_MODEF_PROGRESSIVE, T = RT_MODEF_TEXTURE0, L = RT_MODEF_LINEAR_DISPLAY, A = RT_MODEF_AREA_LIGHTS;
const Want kWant[31] = {
    {"W1E6", "w1e6.wgsl", RT_FAMILY_WORKSHEET1, 0},  {"W6E1", "w6e1.wgsl", RT_FAMILY_PRIMARY, 0},
    {"PROJECT", "project.wgsl", RT_FAMILY_PRIMARY, 0}, {"W7E3", "w7e3.wgsl", RT_FAMILY_PATH, P | A},
    {"W9E1", "w9e1.wgsl", RT_FAMILY_PATH, P},        {"W8E1", "w8e1.wgsl", RT_FAMILY_PATH, P | A},
    {"W8E2", "w8e2.wgsl", RT_FAMILY_PATH, P | A},    {"W8E3", "w8e3.wgsl", RT_FAMILY_PATH, P | A},
    {"W9E2", "w9e2.wgsl", RT_FAMILY_PATH, P},        {"W6E2", "w6e2.wgsl", RT_FAMILY_DIRECT, 0},
    {"W7E1", "w7e1.wgsl", RT_FAMILY_DIRECT, P},      {"W7E2", "w7e2.wgsl", RT_FAMILY_DIRECT, P},
    {"W6E3", "w6e3.wgsl", RT_FAMILY_DIRECT, 0},      {"W9E3", "w9e3.wgsl", RT_FAMILY_PATH, P},
    {"W5E2", "w5e2.wgsl", RT_FAMILY_SWEEP, 0},       {"W5E3", "w5e3.wgsl", RT_FAMILY_SWEEP, 0},
    {"W5E4", "w5e4.wgsl", RT_FAMILY_SWEEP, 0},       {"W5E5", "w5e5.wgsl", RT_FAMILY_SWEEP, 0},
    {"W2E1", "w2e1.wgsl", RT_FAMILY_ANALYTIC, 0},    {"W2E2", "w2e2.wgsl", RT_FAMILY_ANALYTIC, 0},
    {"W2E3", "w2e3.wgsl", RT_FAMILY_ANALYTIC, 0},    {"W2E4", "w2e4.wgsl", RT_FAMILY_ANALYTIC, 0},
    {"W2E5", "w2e5.wgsl", RT_FAMILY_ANALYTIC, 0},    {"W3E1", "w3e1.wgsl", RT_FAMILY_ANALYTIC, T},
    {"W3E2", "w3e2.wgsl", RT_FAMILY_ANALYTIC, T},    {"W3E3", "w3e3.wgsl", RT_FAMILY_ANALYTIC, T},
    {"W3E4", "w3e4.wgsl", RT_FAMILY_ANALYTIC, T},    {"W1E2", "w1e2.wgsl", RT_FAMILY_WORKSHEET1, L},
    {"W1E3", "w1e3.wgsl", RT_FAMILY_WORKSHEET1, L},  {"W1E4", "w1e4.wgsl", RT_FAMILY_WORKSHEET1, 0},
    {"W1E5", "w1e5.wgsl", RT_FAMILY_WORKSHEET1, 0},
};

// the shader files of the 44 scenes (src/scenes.rs) and the rt_mode value each maps to, -1 for none
const struct {
    const char* shader;
    int mode;
} kShaders[] = {
    {"w1e1.wgsl", -1}, {"w1e2.wgsl", 27}, {"w1e3.wgsl", 28}, {"w1e4.wgsl", 29}, {"w1e5.wgsl", 30}, {"w1e6.wgsl", 0},
    {"w2e1.wgsl", 18}, {"w2e2.wgsl", 19}, {"w2e3.wgsl", 20}, {"w2e4.wgsl", 21}, {"w2e5.wgsl", 22}, {"w3e1.wgsl", 23},
    {"w3e2.wgsl", 24}, {"w3e3.wgsl", 25}, {"w3e4.wgsl", 26}, {"w5e2.wgsl", 14}, {"w5e3.wgsl", 15}, {"w5e4.wgsl", 16},
    {"w5e5.wgsl", 17}, {"w6e1.wgsl", 1},  {"w6e2.wgsl", 9},  {"w6e3.wgsl", 12}, {"w7e1.wgsl", 10}, {"w7e2.wgsl", 11},
    {"w7e3.wgsl", 3},  {"w8e1.wgsl", 5},  {"w8e2.wgsl", 6},  {"w8e3.wgsl", 7},  {"w9e1.wgsl", 4},  {"w9e2.wgsl", 8},
    {"w9e3.wgsl", 13}, {"project.wgsl", 2},
};

int bad = 0;
void expect(bool ok, const char* what, int i)
{
    if (ok) return;
    std::printf("MISMATCH %s (%d)\n", what, i);
    bad++;
}

}  // namespace

int main()
{
    static_assert(RT_MODE_COUNT == 31, "the literal table above has 31 rows");
    static_assert(sizeof(rt_mode_desc) == 16 + 2 * sizeof(const char*), "rt_mode_desc: 2 x int32, 2 x uint32, 2 pointers");
    for (int m = -2; m <= RT_MODE_COUNT + 1; m++) {
        rt_mode_desc d;
        std::memset(&d, 0x5A, sizeof d);
        const rt_mode_desc untouched = d;
        const int rc = rt_mode_describe(m, &d);
        if (m < 0 || m >= RT_MODE_COUNT) {
            expect(rc == RT_E_INVALID, "out of range: status", m);
            expect(std::memcmp(&d, &untouched, sizeof d) == 0, "out of range: *out written", m);
            continue;
        }
        const Want& w = kWant[m];
        expect(rc == RT_OK, "status", m);
        expect(d.mode == m && d.family == w.family && d.flags == w.flags && d.reserved == 0, "mode / family / flags", m);
        expect(d.name && std::strcmp(d.name, w.name) == 0, "name", m);
        expect(d.shader && std::strcmp(d.shader, w.shader) == 0, "shader", m);
        expect(rt_mode_describe(m, nullptr) == RT_E_INVALID, "null out", m);
    }
    expect(rt_mode_describe(1000, nullptr) == RT_E_INVALID, "null out, bad mode", 1000);
    int i = 0;
    for (const auto& s : kShaders) {
        const auto d = raytracer::mode_of_shader(s.shader);
        expect(d ? d->mode == s.mode : s.mode == -1, s.shader, i++);
    }
    expect(!raytracer::mode_of_shader(""), "the empty string", 0);
    expect(!raytracer::mode_of_shader(std::string(4096, 'w')), "a 4 KiB string", 0);
    expect(!raytracer::mode_of_shader(std::string("w7e3.wgsl") + std::string(4096, 'x')), "a 4 KiB string with a shader's prefix", 0);
    expect(!raytracer::mode_of_shader("W7E3.WGSL") && !raytracer::mode_of_shader("w7e3"), "near misses", 0);
    std::printf("modes_check: %d mismatches\n", bad);
    return bad ? 1 : 0;
}
