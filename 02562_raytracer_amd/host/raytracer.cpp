// C++ host layer (include/raytracer.hpp) over the C ABI of include/rt.h: the
// reference's Rust host types restated for a C++ caller.  Every GPU action
// goes through rt_* entry points, exactly as the Rust binding of
// INTEGRATION.md would make them.
#include "raytracer.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <sys/stat.h>

namespace raytracer {

// ------------------------------------------------------------------ GpuHandles
GpuHandles::GpuHandles(int device) : device_(device)
{
    const int rc = rt_create(device, &ctx_);
    if (rc != RT_OK) throw Error(rc, "GPUHandles::new: no usable HIP device " + std::to_string(device));
}

GpuHandles::~GpuHandles()
{
    if (ctx_) rt_destroy(ctx_);
}

bool GpuHandles::self_test()
{
    int n = 0;
    return rt_device_count(&n) == RT_OK && n > 0;
}

void GpuHandles::check(int rc, const char* what) const
{
    if (rc != RT_OK) throw Error(rc, std::string(what) + ": " + (ctx_ ? rt_last_error(ctx_) : "no context"));
}

// ------------------------------------------------------------------ camera.rs
Key key_from_name(const std::string& n)
{
    if (n == "W") return Key::W;
    if (n == "A") return Key::A;
    if (n == "S") return Key::S;
    if (n == "D") return Key::D;
    if (n == "Up") return Key::Up;
    if (n == "Down") return Key::Down;
    if (n == "Left") return Key::Left;
    if (n == "Right") return Key::Right;
    return Key::Other;
}

bool CameraController::handle_camera_commands(Key key, bool pressed)
{
    switch (key) {
    case Key::W:
    case Key::Up: forward_ = pressed; return true;
    case Key::A:
    case Key::Left: left_ = pressed; return true;
    case Key::S:
    case Key::Down: backward_ = pressed; return true;
    case Key::D:
    case Key::Right: right_ = pressed; return true;
    default: return false;
    }
}

namespace {
// cgmath's f32 vector operations, in its order of evaluation
inline Vec3 vsub(const Vec3& a, const Vec3& b) { return {a[0] - b[0], a[1] - b[1], a[2] - b[2]}; }
inline Vec3 vadd(const Vec3& a, const Vec3& b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline Vec3 vmul(const Vec3& a, float s) { return {a[0] * s, a[1] * s, a[2] * s}; }
inline float vdot(const Vec3& a, const Vec3& b)
{
    const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    return (x + y) + z;
}
inline float vmag(const Vec3& a) { return std::sqrt(vdot(a, a)); }
inline Vec3 vnormalize(const Vec3& a) { return vmul(a, 1.0f / vmag(a)); }
inline Vec3 vcross(const Vec3& a, const Vec3& b)
{
    return {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
}  // namespace

void CameraController::update_camera(Camera& c) const
{
    const float s = speed_;
    Vec3 forward = vsub(c.target, c.eye);
    const Vec3 forward_norm = vnormalize(forward);
    float forward_mag = vmag(forward);
    if (forward_ && forward_mag > s) c.eye = vadd(c.eye, vmul(forward_norm, s));
    if (backward_) c.eye = vsub(c.eye, vmul(forward_norm, s));
    const Vec3 right = vcross(forward_norm, c.up);
    forward = vsub(c.target, c.eye);
    forward_mag = vmag(forward);
    if (right_) c.eye = vsub(c.target, vmul(vnormalize(vadd(forward, vmul(right, s))), forward_mag));
    if (left_) c.eye = vsub(c.target, vmul(vnormalize(vsub(forward, vmul(right, s))), forward_mag));
}

// ------------------------------------------------------------------ scenes.rs
// kernel_mode() where its row of the mode table passes `keep`
template <class Keep>
static std::optional<rt_mode> mode_if(const std::string& shader, Keep keep)
{
    const auto d = mode_of_shader(shader);
    if (d && keep(*d)) return (rt_mode)d->mode;
    return std::nullopt;
}
static bool walks_tree_or_w1e6(const rt_mode_desc& d) { return RT_FAMILY_NEEDS_TREE(d.family) || d.mode == RT_MODE_W1E6; }

std::optional<rt_mode> SceneDescriptor::kernel_mode() const
{
    return mode_if(shader, [](const rt_mode_desc&) { return true; });
}

std::optional<rt_mode> SceneDescriptor::mode() const { return mode_if(shader, walks_tree_or_w1e6); }

std::optional<rt_mode> SceneDescriptor::render_mode() const
{
    return mode_if(shader, [](const rt_mode_desc& d) { return walks_tree_or_w1e6(d) || d.family == RT_FAMILY_SWEEP; });
}

std::optional<rt_mode> SceneDescriptor::analytic_mode() const
{
    return mode_if(shader, [](const rt_mode_desc& d) { return d.family == RT_FAMILY_ANALYTIC; });
}

std::optional<rt_mode> SceneDescriptor::worksheet1_mode() const
{
    return mode_if(shader, [](const rt_mode_desc& d) { return d.family == RT_FAMILY_WORKSHEET1 && d.mode != RT_MODE_W1E6; });
}

std::vector<SceneDescriptor> get_scenes()
{
    // cameras, scenes.rs:47-85 (aspect comes from the frame)
    auto cam = [](Vec3 e, Vec3 t, Vec3 u, float k) {
        Camera c;
        c.eye = e;
        c.target = t;
        c.up = u;
        c.constant = k;
        return c;
    };
    const Camera basic = cam({2.0f, 1.5f, 2.0f}, {0.0f, 0.5f, 0.0f}, {0.0f, 1.0f, 0.0f}, 1.0f);
    const Camera teapot = cam({0.15f, 1.5f, 10.0f}, {0.15f, 1.5f, 0.0f}, {0.0f, 1.0f, 0.0f}, 2.5f);
    const Camera cornell = cam({277.0f, 275.0f, -570.0f}, {277.0f, 275.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, 1.0f);
    const Camera bunny = cam({-0.02f, 0.11f, 0.6f}, {-0.02f, 0.11f, 0.0f}, {0.0f, 1.0f, 0.0f}, 3.5f);
    const Camera dragon = bunny;   // scenes.rs:79-85 uses the bunny framing
    const std::string campus = "luxo_pxr_campus.jpg", campus_hdr = "luxo_pxr_campus.hdr.png";
    const auto C = VertexType::Combined;
    const auto BSP = TraverseType::Bsp, BVH = TraverseType::Bvh;

    std::vector<SceneDescriptor> v;
    auto S = [&](std::string name, std::string shader, std::optional<std::string> model, const Camera& c,
                 uint32_t w, uint32_t h, VertexType vt = VertexType::Split, TraverseType tt = TraverseType::Bsp,
                 std::optional<std::string> hdri = std::nullopt) {
        SceneDescriptor d;
        d.name = std::move(name);
        d.shader = std::move(shader);
        d.model = std::move(model);
        d.camera = c;
        d.res = {w, h};
        d.vertex_type = vt;
        d.traverse_type = tt;
        d.background_hdri = std::move(hdri);
        v.push_back(std::move(d));
    };
    const int we[15][2] = {{1, 1}, {1, 2}, {1, 3}, {1, 4}, {1, 5}, {1, 6}, {2, 1}, {2, 2},
                           {2, 3}, {2, 4}, {2, 5}, {3, 1}, {3, 2}, {3, 3}, {3, 4}};
    for (const auto& p : we)
        S("W" + std::to_string(p[0]) + " E" + std::to_string(p[1]),
          "w" + std::to_string(p[0]) + "e" + std::to_string(p[1]) + ".wgsl", std::nullopt, basic, 512, 512);
    S("W5 E2 Teapot", "w5e2.wgsl", "teapot.obj", teapot, 800, 450);
    S("W5 E3 Teapot", "w5e3.wgsl", "teapot.obj", teapot, 800, 450);
    S("W5 E4 Cornell Box", "w5e4.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512);
    S("W5 E5 Cornell Box", "w5e5.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512);
    S("W6 E1 Teapot", "w6e1.wgsl", "teapot.obj", teapot, 800, 450);
    S("W6 E1 Bunny", "w6e1.wgsl", "bunny.obj", bunny, 512, 512);
    S("W6 E1 Dragon", "w6e1.wgsl", "dragon.obj", dragon, 800, 450);
    S("W6 E2 Cornell Box", "w6e2.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512, C);
    S("W6 E3 Cornell Box", "w6e3.wgsl", "CornellBox.obj", cornell, 512, 512, C);
    S("W7 E1 Cornell Box", "w7e1.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512, C);
    S("W7 E2 Cornell Box", "w7e2.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512, C);
    S("W7 E3 Cornell Box", "w7e3.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512, C);
    S("W8 E1 Cornell Box Balls", "w8e1.wgsl", "CornellBox.obj", cornell, 512, 512, C);
    S("W8 E2 Cornell Box Balls", "w8e2.wgsl", "CornellBox.obj", cornell, 512, 512, C);
    S("W8 E3 Absorption", "w8e3.wgsl", "CornellBox.obj", cornell, 512, 512, C);
    S("W9 E1 Teapot", "w9e1.wgsl", "teapot.obj", teapot, 800, 450, C, BSP, campus);
    S("W9 E1 Bunny", "w9e1.wgsl", "bunny.obj", bunny, 512, 512, C, BSP, campus);
    S("W9 E2 Teapot", "w9e2.wgsl", "teapot.obj", teapot, 800, 450, C, BSP, campus_hdr);
    S("W9 E2 Bunny", "w9e2.wgsl", "bunny.obj", bunny, 512, 512, C, BSP, campus_hdr);
    S("W9 E3 Teapot", "w9e3.wgsl", "teapot.obj", teapot, 800, 450, C, BSP, campus);
    S("Project: Quad", "project.wgsl", "plane.obj", basic, 512, 512, C, BVH);
    S("Project: Three Quads", "project.wgsl", "test_object.obj", basic, 512, 512, C, BVH);
    S("Project: Cornell Box", "project.wgsl", "CornellBoxWithBlocks.obj", cornell, 512, 512, C, BVH);
    S("Project: Utah Teapot", "project.wgsl", "teapot.obj", teapot, 800, 450, C, BVH);
    S("Project: Utah Teapot BSP", "project.wgsl", "teapot.obj", teapot, 800, 450, C, BSP);
    S("Project: Bunny", "project.wgsl", "bunny.obj", bunny, 512, 512, C, BVH);
    S("Project: Bunny BSP", "project.wgsl", "bunny.obj", bunny, 512, 512, C, BSP);
    S("Project: Dragon", "project.wgsl", "dragon.obj", dragon, 800, 450, C, BVH);
    S("Project: Dragon BSP", "project.wgsl", "dragon.obj", dragon, 800, 450, C, BSP);
    return v;
}

const SceneDescriptor& find_scene(const std::string& name)
{
    static const std::vector<SceneDescriptor> table = get_scenes();
    for (const auto& s : table)
        if (s.name == name) return s;
    throw Error(RT_E_INVALID, "no scene named '" + name + "'");
}

// ------------------------------------------------------------------ uniform.rs
Lcg64Xsh32::Lcg64Xsh32(uint64_t state, uint64_t stream)
{
    increment_ = (stream << 1) | 1u;
    state_ = state + increment_;
    state_ = state_ * 6364136223846793005ull + increment_;
}

uint32_t Lcg64Xsh32::next_u32()
{
    const uint64_t s = state_;
    state_ = state_ * 6364136223846793005ull + increment_;
    const uint32_t rot = (uint32_t)(s >> 59);
    const uint32_t xsh = (uint32_t)(((s >> 18) ^ s) >> 27);
    return (xsh >> rot) | (xsh << ((32u - rot) & 31u));
}

uint64_t Lcg64Xsh32::next_u64()
{
    const uint64_t lo = next_u32();
    const uint64_t hi = next_u32();
    return (hi << 32) | lo;
}

double Lcg64Xsh32::gen_unit_f64()
{
    const uint64_t bits = (next_u64() >> 12) | 0x3FF0000000000000ull;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v - 1.0;
}

std::vector<std::array<float, 2>> compute_jitters(double pixel_size, uint32_t subdivs)
{
    if (subdivs == 0 || subdivs > MAX_SUBDIVISION || pixel_size == 0.0)
        throw Error(RT_E_INVALID, "compute_jitters: subdivs must be in 1..10 and pixel_size nonzero");
    std::vector<std::array<float, 2>> out;
    if (subdivs == 1) {
        out.push_back({0.0f, 0.0f});
        return out;
    }
    Lcg64Xsh32 rng(0, 0);
    const double step = pixel_size / subdivs;
    for (uint32_t i = 0; i < subdivs; i++)
        for (uint32_t j = 0; j < subdivs; j++) {
            const double u1 = rng.gen_unit_f64();
            const double u2 = rng.gen_unit_f64();
            out.push_back({(float)((u1 + j) * step - pixel_size * 0.5), (float)((u2 + i) * step - pixel_size * 0.5)});
        }
    return out;
}

rt_uniform make_uniform(const Camera& cam, uint32_t width, uint32_t height, uint32_t selection1,
                        uint32_t subdivision_level, uint32_t iteration, uint32_t selection2, uint32_t use_texture,
                        std::array<float, 2> uv_scale)
{
    rt_uniform u;
    std::memset(&u, 0, sizeof u);
    for (int i = 0; i < 3; i++) {
        u.camera_pos[i] = cam.eye[i];
        u.camera_look_at[i] = cam.target[i];
        u.camera_up[i] = cam.up[i];
    }
    u.camera_constant = cam.constant;
    u.aspect_ratio = (float)width / (float)height;   // headless: the frame's W/H (render_state.rs:563-566)
    u.selection1 = selection1;
    u.selection2 = selection2;
    u.subdivision_level = subdivision_level;
    u.use_texture = use_texture;
    u.iteration = iteration;
    u.uv_scale[0] = uv_scale[0];
    u.uv_scale[1] = uv_scale[1];
    u.resolution[0] = width;
    u.resolution[1] = height;
    return u;
}

std::vector<uint8_t> synth_texture(uint32_t size)
{
    std::vector<uint8_t> t((size_t)size * size * 4);
    for (uint32_t y = 0; y < size; y++)
        for (uint32_t x = 0; x < size; x++) {
            uint32_t h = (x * 73856093u) ^ (y * 19349663u);
            h = (h ^ (h >> 13)) * 0x5BD1E995u;
            h = h ^ (h >> 15);
            uint8_t* p = &t[((size_t)y * size + x) * 4];
            p[0] = (uint8_t)(40u + (h & 63u));
            p[1] = (uint8_t)(120u + ((h >> 8) & 127u));
            p[2] = (uint8_t)(20u + ((h >> 16) & 31u));
            p[3] = 255;
        }
    return t;
}

// ------------------------------------------------------------------ mesh.rs
Mesh Mesh::load(const std::string& path)
{
    rt_mesh_host* m = nullptr;
    const int rc = rt_mesh_load_obj(path.c_str(), &m);
    if (rc != RT_OK) throw Error(rc, "Mesh::from_obj: cannot load " + path);
    return Mesh(m);
}

Mesh Mesh::synth_bunny(uint32_t ntris, uint32_t seed)
{
    rt_mesh_host* m = nullptr;
    const int rc = rt_mesh_synth_bunny(ntris, seed, &m);
    if (rc != RT_OK) throw Error(rc, "synth_bunny failed");
    return Mesh(m);
}

Mesh::~Mesh()
{
    if (m_) rt_mesh_free(m_);
}

uint32_t Mesh::ntris() const
{
    rt_mesh_view v;
    if (rt_mesh_view_get(m_, &v) != RT_OK) return 0;
    return v.ntris;
}

// ------------------------------------------------------------------ render_state.rs
RenderState::RenderState(GpuHandles& gpu, const SceneDescriptor& scene, RenderOptions opts)
    : gpu_(gpu), opts_(std::move(opts))
{
    setup_rendering(scene);
}

RenderState::~RenderState() { release(); }

void RenderState::release()
{
    // deregister before free: the context never keeps a pointer into a buffer that is gone
    if (counts_) rt_set_adaptive(gpu_.ctx(), nullptr, 0.0f, 0.0f, 0, 0);
    if (noise_) rt_set_noise_buffer(gpu_.ctx(), nullptr);
    accum_.reset();
    ids_.reset();
    tile_accum_.reset();
    tile_ids_.reset();
    counts_.reset();
    noise_.reset();
    disable_temporal();
}

// the k_path modes (rt.h "noise estimate")
static bool writes_records(const rt_mode_desc& row) { return row.family == RT_FAMILY_PATH; }

void RenderState::enable_noise()
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, "enable_noise is for an untiled state: a tiled render (set_tiling, any rank count) keeps its states packed per tile");
    if (!writes_records(row_))
        throw Error(RT_E_UNSUPPORTED, "enable_noise: the mode writes no per-iteration records");
    if (iteration_) throw Error(RT_E_INVALID, "enable_noise: the estimate starts at iteration 0");
    if (!noise_) {   // a member only once it is cleared: a failed clear leaves the estimate off
        DeviceArray<rt_noise_state> fresh(gpu_, (size_t)width_ * height_, "noise buffer");
        fresh.zero("clear noise buffer");
        noise_ = std::move(fresh);
    }
    gpu_.check(rt_set_noise_buffer(gpu_.ctx(), noise_.get()), "set noise buffer");
}

std::vector<float> RenderState::noise_map(float floor) const
{
    if (!noise_) throw Error(RT_E_NOT_READY, "noise_map: enable_noise() first");
    if (tiled_) throw Error(RT_E_UNSUPPORTED, "noise_map is for an untiled state: a tiled render (set_tiling, any rank count) keeps its states packed per tile");
    const DeviceArray<float> d(gpu_, noise_.size(), "noise map buffer");
    gpu_.check(rt_noise_map(gpu_.ctx(), noise_.get(), (uint32_t)noise_.size(), iteration_, floor, d.get()), "noise_map");
    return d.download("noise_map");
}

rt_noise_summary RenderState::noise_summary(float threshold, float floor) const
{
    if (!noise_) throw Error(RT_E_NOT_READY, "noise_summary: enable_noise() first");
    if (tiled_) throw Error(RT_E_UNSUPPORTED, "noise_summary is for an untiled state: a tiled render (set_tiling, any rank count) keeps its states packed per tile");
    rt_noise_summary s;
    gpu_.check(rt_noise_summarize(gpu_.ctx(), noise_.get(), (uint32_t)noise_.size(), iteration_, threshold, floor, &s),
               "noise_summary");
    return s;
}

uint32_t RenderState::render_until(float target, uint32_t max_samples, uint32_t batch, double allow, float floor,
                                   rt_noise_summary* summary)
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, "render_until is for an untiled state: a tiled render (set_tiling, any rank count) keeps its states packed per tile");
    if (!progressive_) throw Error(RT_E_INVALID, "render_until needs progressive rendering");
    if (batch == 0) throw Error(RT_E_INVALID, "render_until: batch must be at least 1");
    if (!noise_) enable_noise();
    rt_noise_summary s{};
    while (iteration_ < max_samples) {
        render(std::min(batch, max_samples - iteration_));
        if (iteration_ >= 2) {
            s = noise_summary(target, floor);
            if ((double)s.above <= allow * (double)s.pixels) break;
        }
    }
    if (summary) *summary = s;
    return iteration_;
}

static const char* const kAdaptiveUntiled =
    " is for an untiled state: a tiled render (set_tiling, any rank count) keeps its counts packed per tile";

void RenderState::enable_adaptive(float target, float floor, uint32_t min_samples, int vote)
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("enable_adaptive") + kAdaptiveUntiled);
    if (!writes_records(row_))
        throw Error(RT_E_UNSUPPORTED, "enable_adaptive: the mode writes no per-iteration records");
    if (iteration_) throw Error(RT_E_INVALID, "enable_adaptive: the counts start at iteration 0");
    if (min_samples < 2 || !(target >= 0.0f) || !(floor > 0.0f) || (vote != RT_ADAPT_PIXEL && vote != RT_ADAPT_TILE))
        throw Error(RT_E_INVALID, "enable_adaptive: min_samples >= 2, target >= 0, floor > 0, vote pixel or tile");
    if (!noise_) enable_noise();
    if (!counts_) {   // as the noise buffer: a member only once it is cleared
        DeviceArray<uint32_t> fresh(gpu_, (size_t)width_ * height_, "sample count buffer");
        fresh.zero("clear sample counts");
        counts_ = std::move(fresh);
    }
    ad_target_ = target;
    ad_floor_ = floor;
    ad_min_ = min_samples;
    ad_vote_ = vote;
    gpu_.check(rt_set_adaptive(gpu_.ctx(), counts_.get(), target, floor, min_samples, vote), "set adaptive");
}

std::vector<uint32_t> RenderState::sample_counts() const
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("sample_counts") + kAdaptiveUntiled);
    if (!counts_) throw Error(RT_E_NOT_READY, "sample_counts: enable_adaptive() first");
    return counts_.download("sample_counts");
}

rt_adaptive_summary RenderState::adaptive_summary() const
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("adaptive_summary") + kAdaptiveUntiled);
    if (!counts_) throw Error(RT_E_NOT_READY, "adaptive_summary: enable_adaptive() first");
    rt_adaptive_summary s;
    gpu_.check(rt_adaptive_summarize(gpu_.ctx(), noise_.get(), counts_.get(), width_, height_, iteration_, ad_target_,
                                     ad_floor_, ad_min_, ad_vote_, &s),
               "adaptive_summary");
    return s;
}

uint32_t RenderState::render_adaptive(uint32_t max_samples, uint32_t batch, rt_adaptive_summary* summary)
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("render_adaptive") + kAdaptiveUntiled);
    if (!counts_) throw Error(RT_E_NOT_READY, "render_adaptive: enable_adaptive() first");
    if (!progressive_) throw Error(RT_E_INVALID, "render_adaptive needs progressive rendering");
    if (batch == 0) throw Error(RT_E_INVALID, "render_adaptive: batch must be at least 1");
    rt_adaptive_summary s{};
    while (iteration_ < max_samples) {
        render(std::min(batch, max_samples - iteration_));
        s = adaptive_summary();
        if (s.live_next == 0) break;
    }
    if (summary) *summary = s;
    return iteration_;
}

// the packed tile buffers of one rank for a width x height frame (zeroed: the accumulation
// of iteration 0 is not read), both or neither
static void make_tiles(const GpuHandles& gpu, uint32_t width, uint32_t height, uint32_t nranks,
                       DeviceArray<float>& accum, DeviceArray<uint32_t>& ids)
{
    const size_t px = (size_t)rt_tileset_local_tiles(width, height, nranks) * 64u;
    DeviceArray<float> a(gpu, px * 4, "tile accumulation buffer");
    DeviceArray<uint32_t> i(gpu, px, "tile id buffer");
    a.zero("clear tile accumulation");
    accum = std::move(a);
    ids = std::move(i);
}

void RenderState::set_tiling(uint32_t nranks, uint32_t rank, const uint8_t comm_id[RT_COMM_ID_BYTES])
{
    if (tiled_) throw Error(RT_E_INVALID, "set_tiling: already tiled");
    if (counts_) throw Error(RT_E_UNSUPPORTED, "set_tiling: adaptive sampling is enabled (it is for an untiled state)");
    // the noise buffer is width x height states, row-major; tile renders would write it packed per tile
    if (noise_) throw Error(RT_E_UNSUPPORTED, "set_tiling: the noise estimate is enabled (it is for an untiled state)");
    if (temporal_) throw Error(RT_E_UNSUPPORTED, "set_tiling: temporal accumulation is enabled (it is for an untiled state)");
    gpu_.check(rt_comm_init(gpu_.ctx(), nranks, rank, comm_id), "communicator");
    make_tiles(gpu_, width_, height_, nranks, tile_accum_, tile_ids_);   // (a throw leaves the state untiled)
    nranks_ = nranks;
    rank_ = rank;
    tiled_ = true;
}

void RenderState::setup_rendering(const SceneDescriptor& scene)
{
    const auto row = mode_of_shader(scene.shader);
    if (!row) throw Error(RT_E_UNSUPPORTED, scene.shader + " is outside the hot path (SURVEY.md section 2)");
    scene_ = scene;
    camera_ = scene.camera;
    row_ = *row;
    width_ = opts_.resolution ? opts_.resolution->first : scene.res.first;
    height_ = opts_.resolution ? opts_.resolution->second : scene.res.second;
    rt_ctx* c = gpu_.ctx();
    const bool tree = RT_FAMILY_NEEDS_TREE(row_.family);
    trav_ = !tree ? RT_TRAVERSE_NONE : scene.traverse_type == TraverseType::Bsp ? RT_TRAVERSE_BSP : RT_TRAVERSE_BVH;
    if (row_.flags & RT_MODEF_TEXTURE0) {
        // the W3 scenes sample texture0 (grass.jpg is not redistributed and this layer
        // decodes no JPEG: the stand-in, or set_texture_image)
        const auto tex = synth_texture();
        gpu_.check(rt_set_texture(c, tex.data(), 64, 64), "texture0");
    } else if (row_.family == RT_FAMILY_ANALYTIC) {
        gpu_.check(rt_set_texture(c, nullptr, 0, 0), "texture0");
    }
    if (RT_FAMILY_NEEDS_MESH(row_.family)) {
        const std::string path = opts_.models_dir + "/" + scene.model.value_or("");
        struct stat st;
        const bool exists = ::stat(path.c_str(), &st) == 0;
        Mesh mesh = (!exists && scene.model == std::string("bunny.obj") && opts_.bunny_standin) ? Mesh::synth_bunny()
                                                                                                 : Mesh::load(path);
        gpu_.check(rt_upload_mesh_host(c, mesh.get()), "upload mesh");
        if (trav_ == RT_TRAVERSE_BSP) {
            if (opts_.device_build) {
                gpu_.check(rt_build_bsp_device(c, 20, 4, nullptr), "BSP device build");
            } else {   // Mesh::bsp_tree, mesh.rs:229-231 (depth 20, leaf 4)
                rt_bsp_host* b = nullptr;
                gpu_.check(rt_bsp_build(mesh.get(), 20, 4, 0, &b), "BSP build");
                const std::unique_ptr<rt_bsp_host, decltype(&rt_bsp_free)> own(b, rt_bsp_free);
                gpu_.check(rt_upload_bsp_host(c, b), "upload BSP");
            }
        } else if (trav_ == RT_TRAVERSE_BVH) {   // (NONE: the brute-force W5 scenes, the mesh alone)
            if (opts_.device_build) {
                gpu_.check(rt_build_bvh_device(c, 4, nullptr), "HLBVH device build");
            } else {   // Mesh::bvh, mesh.rs:233-239 (leaf 4)
                rt_bvh_host* b = nullptr;
                gpu_.check(rt_bvh_build(mesh.get(), 4, &b), "HLBVH build");
                const std::unique_ptr<rt_bvh_host, decltype(&rt_bvh_free)> own(b, rt_bvh_free);
                gpu_.check(rt_upload_bvh_host(c, b), "upload BVH");
            }
        }
    }
    gpu_.check(rt_set_environment(c, opts_.environment.data()), "environment");
    gpu_.check(rt_set_environment_map(c, nullptr, 0, 0), "environment map");
    const bool had_noise = (bool)noise_, had_adaptive = (bool)counts_, had_temporal = temporal_;
    release();   // free, then allocate: the old frame and the new need not fit side by side
    const size_t npx = (size_t)width_ * height_;
    accum_ = DeviceArray<float>(gpu_, npx * 4, "accumulation buffer");
    ids_ = DeviceArray<uint32_t>(gpu_, npx, "id buffer");
    accum_.zero("clear accumulation");
    if (tiled_) make_tiles(gpu_, width_, height_, nranks_, tile_accum_, tile_ids_);
    iteration_ = 0;
    if (had_noise && writes_records(row_)) enable_noise();   // the buffer follows the scene
    if (had_adaptive && writes_records(row_)) enable_adaptive(ad_target_, ad_floor_, ad_min_, ad_vote_);
    if (had_temporal && writes_records(row_)) enable_temporal(tp_max_history_, tp_normal_min_, tp_plane_tol_, tp_min_len_);
    update();
}

void RenderState::load_scene(const SceneDescriptor& scene)
{
    iteration_ = 0;
    setup_rendering(scene);
}

void RenderState::update()
{
    camera_.aspect = (float)width_ / (float)height_;
    controller_.update_camera(camera_);
    uniform_ = make_uniform(camera_, width_, height_, selection1_, subdivision_, iteration_, selection2_, use_texture_,
                            uv_scale_);
    const auto jit = compute_jitters(1.0 / (double)height_, subdivision_);
    gpu_.check(rt_set_uniforms(gpu_.ctx(), &uniform_, &jit[0][0]), "set uniforms");
}

void RenderState::render(uint32_t spp)
{
    if (tiled_) {
        // this rank's tiles, then every rank's tiles into rank 0's frame
        const rt_tileset ts{rank_, nranks_};
        gpu_.check(rt_render_tiles(gpu_.ctx(), mode(), trav_, &ts, iteration_, spp, tile_accum_.get(), tile_ids_.get(), nullptr),
                   "render tiles");
        const bool root = rank_ == 0;
        gpu_.check(rt_gather_tiles(gpu_.ctx(), width_, height_, tile_accum_.get(), tile_ids_.get(),
                                   root ? accum_.get() : nullptr, root ? ids_.get() : nullptr),
                   "gather tiles");
    } else {
        const rt_tile region{0, 0, width_, height_};
        gpu_.check(rt_render(gpu_.ctx(), mode(), trav_, &region, iteration_, spp, accum_.get(), ids_.get(), nullptr), "render");
    }
    if (progressive_ && (row_.flags & RT_MODEF_PROGRESSIVE)) iteration_ += spp;
    update();
}

bool RenderState::step()
{
    if (progressive_ && iteration_ >= max_iterations_) return false;
    render(1);
    return true;
}

bool RenderState::input_alt(Key key, bool pressed) { return controller_.handle_camera_commands(key, pressed); }
void RenderState::update_camera_constant(float constant) { camera_.constant = constant; }

void RenderState::set_samples(uint32_t samples, bool enabled)
{
    progressive_ = enabled;
    max_iterations_ = enabled ? samples : 2;
}

void RenderState::set_subdivision_level(uint32_t level) { subdivision_ = level <= MAX_SUBDIVISION ? level : MAX_SUBDIVISION; }
void RenderState::set_selection1(uint32_t shader) { selection1_ = shader; }

void RenderState::set_other_material(uint32_t shader) { selection2_ = shader; }
void RenderState::set_texture(uint32_t use_texture, std::array<float, 2> uv_scale)
{
    use_texture_ = use_texture;
    uv_scale_ = uv_scale;
}
void RenderState::set_texture_image(const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    gpu_.check(rt_set_texture(gpu_.ctx(), rgba8, width, height), "texture0");
}

void RenderState::set_environment_map(const uint8_t* rgba8, uint32_t width, uint32_t height)
{
    gpu_.check(rt_set_environment_map(gpu_.ctx(), rgba8, width, height), "environment map");
}

void RenderState::reset_iteration()
{
    iteration_ = 0;
    update();
}

std::vector<float> RenderState::frame() const { return accum_.download("download frame"); }
std::vector<uint32_t> RenderState::hit_ids() const { return ids_.download("download ids"); }

// a float4 frame on the device as the sRGB surface would hold it (rt_frame_rgba8_mode)
static std::vector<uint8_t> rgba8_of(const GpuHandles& gpu, rt_mode mode, const DeviceArray<float>& frame, const char* what)
{
    const DeviceArray<uint8_t> img(gpu, frame.size(), what);
    gpu.check(rt_frame_rgba8_mode(gpu.ctx(), mode, frame.get(), (uint32_t)(frame.size() / 4), img.get()), what);
    return img.download(what);
}

std::vector<uint8_t> RenderState::frame_rgba8() const { return rgba8_of(gpu_, mode(), accum_, "frame_rgba8"); }

// ---- the guide with objects (rt.h "denoise / Guide with objects")
// Its entry points are referenced weakly, so that this file also links against a library from
// before they existed (and against a test's stub of the ABI): absent, the flag's first use throws
// RT_E_UNSUPPORTED and everything else works as before.
extern "C" {
int rt_guide_objects(int mode, uint32_t* objects) __attribute__((weak));
int rt_denoise_guide_objects(rt_ctx* ctx, uint32_t objects, uint32_t width, uint32_t height, const uint32_t* ids_dev,
                             float* nz_dev, float* dz_dev) __attribute__((weak));
int rt_denoise_objects(rt_ctx* ctx, uint32_t objects, uint32_t width, uint32_t height, const float* accum_dev,
                       const uint32_t* ids_dev, const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t n,
                       uint32_t levels, float sigma_l, float sigma_z, float* out_rgba_dev) __attribute__((weak));
}

void RenderState::set_guide_objects(bool on)
{
    if (temporal_)
        throw Error(RT_E_UNSUPPORTED, "set_guide_objects: temporal accumulation is enabled and its history holds the guide it "
                                      "was made with (set_guide_objects before enable_temporal)");
    guide_objects_ = on;
}

// the objects mask of the guides this state makes; 0: rt_denoise_guide and rt_denoise themselves
uint32_t RenderState::guide_mask(const char* who) const
{
    if (!guide_objects_) return 0;
    if (!rt_guide_objects || !rt_denoise_guide_objects || !rt_denoise_objects)
        throw Error(RT_E_UNSUPPORTED, std::string(who) + ": set_guide_objects is on, and the library has no rt_denoise_guide_objects");
    uint32_t objects = 0;
    gpu_.check(rt_guide_objects(mode(), &objects), who);
    return objects;
}

// the denoised frame on the device
DeviceArray<float> RenderState::denoise_device(uint32_t levels, float sigma_l, float sigma_z) const
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, "denoise is for an untiled state: the filter needs every pixel's neighbours, and a tiled render (set_tiling, any rank count) keeps its buffers packed per tile");
    if (!writes_records(row_)) throw Error(RT_E_UNSUPPORTED, "denoise: the mode keeps no noise state");
    if (!noise_) throw Error(RT_E_NOT_READY, "denoise: enable_noise() first");
    if (iteration_ < 2) throw Error(RT_E_INVALID, "denoise: the variance needs at least 2 rendered iterations");
    if (levels < 1 || levels > 5 || !(sigma_l > 0.0f) || !(sigma_z > 0.0f))
        throw Error(RT_E_INVALID, "denoise: levels in 1..5, sigmas > 0");
    const uint32_t objects = guide_mask("denoise");
    DeviceArray<float> d(gpu_, accum_.size(), "denoise buffer");
    gpu_.check(objects ? rt_denoise_objects(gpu_.ctx(), objects, width_, height_, accum_.get(), ids_.get(), noise_.get(),
                                            counts_.get(), iteration_, levels, sigma_l, sigma_z, d.get())
                       : rt_denoise(gpu_.ctx(), width_, height_, accum_.get(), ids_.get(), noise_.get(), counts_.get(),
                                    iteration_, levels, sigma_l, sigma_z, d.get()),
               "denoise");
    return d;
}

std::vector<float> RenderState::denoise(uint32_t levels, float sigma_l, float sigma_z) const
{
    return denoise_device(levels, sigma_l, sigma_z).download("denoise");
}

std::vector<uint8_t> RenderState::denoised_rgba8(uint32_t levels, float sigma_l, float sigma_z) const
{
    return rgba8_of(gpu_, mode(), denoise_device(levels, sigma_l, sigma_z), "denoised_rgba8");
}

// ---- temporal accumulation (rt.h "temporal accumulation")
static const char* const kTemporalUntiled =
    " is for an untiled state: reprojection needs every pixel's neighbours, and a tiled render (set_tiling, any rank "
    "count) keeps its buffers packed per tile";

void RenderState::enable_temporal(uint32_t max_history, float normal_min, float plane_tol, uint32_t min_len)
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("enable_temporal") + kTemporalUntiled);
    if (!writes_records(row_))
        throw Error(RT_E_UNSUPPORTED, "enable_temporal: the mode writes no per-iteration records (a path mode only)");
    if (max_history < 1 || min_len < 1 || !(plane_tol >= 0.0f) || normal_min != normal_min)
        throw Error(RT_E_INVALID, "enable_temporal: max_history and min_len >= 1, plane_tol >= 0, normal_min a number");
    disable_temporal();
    const size_t npx = (size_t)width_ * height_;
    // into locals: a failed allocation leaves the state off, with nothing held
    DeviceArray<float> cur(gpu_, npx * 4, "temporal frame buffer");
    DeviceArray<uint32_t> ids(gpu_, npx, "temporal id buffer");
    DeviceArray<float> dz(gpu_, npx * 2, "temporal guide buffer");
    TemporalSet set[2];
    for (TemporalSet& s : set) {
        s.color = DeviceArray<float>(gpu_, npx * 4, "temporal history colour");
        s.mom = DeviceArray<float>(gpu_, npx * 2, "temporal history moments");
        s.len = DeviceArray<uint32_t>(gpu_, npx, "temporal history length");
        s.nz = DeviceArray<float>(gpu_, npx * 4, "temporal history guide");
    }
    tp_cur_ = std::move(cur);
    tp_ids_ = std::move(ids);
    tp_dz_ = std::move(dz);
    for (int i = 0; i < 2; i++) tp_set_[i] = std::move(set[i]);
    temporal_ = true;
    tp_max_history_ = max_history;
    tp_normal_min_ = normal_min;
    tp_plane_tol_ = plane_tol;
    tp_min_len_ = min_len;
    tp_latest_ = -1;
    tp_k_ = 0;
}

void RenderState::disable_temporal()
{
    tp_cur_.reset();
    tp_ids_.reset();
    tp_dz_.reset();
    for (TemporalSet& s : tp_set_) s = TemporalSet{};
    temporal_ = false;
    tp_latest_ = -1;
}

void RenderState::temporal_step(uint32_t spp)
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("temporal_step") + kTemporalUntiled);
    if (!temporal_) throw Error(RT_E_NOT_READY, "temporal_step: enable_temporal() first");
    if (spp < 1) throw Error(RT_E_INVALID, "temporal_step: spp must be at least 1");
    const uint32_t objects = guide_mask("temporal_step");
    rt_ctx* c = gpu_.ctx();
    tp_cur_.zero("clear temporal frame");
    // the frame is not the progressive render's: its noise state and counts stay as they are.  Both
    // registrations come back whatever happened, and the first failure is the one reported
    int rc = RT_OK;
    const auto then = [&rc](int r) { rc = rc == RT_OK ? r : rc; };
    if (counts_) rc = rt_set_adaptive(c, nullptr, 0.0f, 0.0f, 0, 0);
    if (noise_) then(rt_set_noise_buffer(c, nullptr));
    const rt_tile region{0, 0, width_, height_};
    if (rc == RT_OK) rc = rt_render(c, mode(), trav_, &region, tp_k_, spp, tp_cur_.get(), tp_ids_.get(), nullptr);
    if (noise_) then(rt_set_noise_buffer(c, noise_.get()));
    if (counts_) then(rt_set_adaptive(c, counts_.get(), ad_target_, ad_floor_, ad_min_, ad_vote_));
    gpu_.check(rc, "temporal render");
    // an empty set's buffers are null: the first frame has no history
    const TemporalSet none, &old = tp_latest_ < 0 ? none : tp_set_[tp_latest_];
    const TemporalSet& out = tp_set_[tp_latest_ < 0 ? 0 : 1 - tp_latest_];
    // the guide of the camera that rendered the frame: before update() moves it
    gpu_.check(objects ? rt_denoise_guide_objects(c, objects, width_, height_, tp_ids_.get(), out.nz.get(), tp_dz_.get())
                       : rt_denoise_guide(c, width_, height_, tp_ids_.get(), out.nz.get(), tp_dz_.get()),
               "temporal guide");
    const float scale = (float)(tp_k_ + spp) / (float)spp;
    gpu_.check(rt_temporal_accumulate(c, width_, height_, tp_cur_.get(), scale, out.nz.get(),
                                      tp_latest_ < 0 ? nullptr : &tp_uniform_, old.color.get(), old.mom.get(), old.len.get(),
                                      old.nz.get(), tp_max_history_, tp_normal_min_, tp_plane_tol_, out.color.get(),
                                      out.mom.get(), out.len.get()),
               "temporal accumulate");
    tp_latest_ = tp_latest_ < 0 ? 0 : 1 - tp_latest_;
    tp_uniform_ = uniform_;
    tp_k_ += spp;
    update();
}

// the filtered latest frame on the device
DeviceArray<float> RenderState::temporal_device(uint32_t levels, float sigma_l, float sigma_z) const
{
    if (tiled_) throw Error(RT_E_UNSUPPORTED, std::string("temporal_frame") + kTemporalUntiled);
    if (!temporal_ || tp_latest_ < 0) throw Error(RT_E_NOT_READY, "temporal_frame: enable_temporal() and temporal_step() first");
    if (levels < 1 || levels > 5 || !(sigma_l > 0.0f) || !(sigma_z > 0.0f))
        throw Error(RT_E_INVALID, "temporal_frame: levels in 1..5, sigmas > 0");
    rt_ctx* c = gpu_.ctx();
    const size_t npx = (size_t)width_ * height_;
    const TemporalSet& s = tp_set_[tp_latest_];
    const DeviceArray<float> var(gpu_, npx, "temporal variance buffer");
    DeviceArray<float> d(gpu_, npx * 4, "temporal_frame");
    gpu_.check(rt_temporal_variance(c, width_, height_, s.mom.get(), s.len.get(), s.nz.get(), tp_dz_.get(), tp_min_len_,
                                    tp_normal_min_, tp_plane_tol_, var.get()),
               "temporal_frame");
    gpu_.check(rt_denoise_filter(c, width_, height_, s.color.get(), var.get(), s.nz.get(), tp_dz_.get(), levels, sigma_l,
                                 sigma_z, d.get(), nullptr),
               "temporal_frame");
    gpu_.check(rt_synchronize(c), "temporal_frame");   // the filter reads var, which goes here
    return d;
}

std::vector<float> RenderState::temporal_frame(uint32_t levels, float sigma_l, float sigma_z) const
{
    return temporal_device(levels, sigma_l, sigma_z).download("temporal_frame");
}

std::vector<uint8_t> RenderState::temporal_rgba8(uint32_t levels, float sigma_l, float sigma_z) const
{
    return rgba8_of(gpu_, mode(), temporal_device(levels, sigma_l, sigma_z), "temporal_rgba8");
}

RenderState::TemporalCurrent RenderState::temporal_current() const
{
    if (!temporal_ || tp_latest_ < 0) throw Error(RT_E_NOT_READY, "temporal_current: enable_temporal() and temporal_step() first");
    TemporalCurrent cur;
    cur.accum = tp_cur_.download("download temporal frame");
    cur.ids = tp_ids_.download("download temporal ids");
    cur.uniform = tp_uniform_;
    return cur;
}

RenderState::TemporalHistory RenderState::temporal_history() const
{
    if (!temporal_ || tp_latest_ < 0) throw Error(RT_E_NOT_READY, "temporal_history: enable_temporal() and temporal_step() first");
    const TemporalSet& s = tp_set_[tp_latest_];
    TemporalHistory h;
    h.color = s.color.download("download temporal colour");
    h.moments = s.mom.download("download temporal moments");
    h.length = s.len.download("download temporal length");
    return h;
}

rt_ray_counts RenderState::last_counts() const
{
    rt_ray_counts c;
    gpu_.check(rt_last_counts(gpu_.ctx(), &c), "counts");
    return c;
}

}  // namespace raytracer
