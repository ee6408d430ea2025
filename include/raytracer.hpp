/* C++ host layer of the drop-in: the reference's Rust host types above its
 * GPU boundary (src/gpu_handles.rs, src/scenes.rs, src/camera.rs,
 * src/bindings/uniform.rs, src/render_state.rs, the progressive loop of
 * src/lib.rs:321-489), restated in C++ over the C ABI of include/rt.h -- the
 * calls a Rust host would make through its extern "C" block.
 *
 * Headless: no window, surface or egui panel.  A RenderState renders into an
 * HBM RGBA32F accumulation buffer (the RenderDestination texture) and hands
 * back the linear accumulation, the primary-hit ids and the sRGB frame.
 * Errors from the C ABI surface as raytracer::Error (code + rt_last_error).
 */
#pragma once

#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rt.h"

namespace raytracer {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code(code) {}
    int code;
};

/* ---- src/gpu_handles.rs: the device + stream wrapper (GPUHandles::new, self_test) */
class GpuHandles {
public:
    explicit GpuHandles(int device = 0);
    ~GpuHandles();
    GpuHandles(const GpuHandles&) = delete;
    GpuHandles& operator=(const GpuHandles&) = delete;
    rt_ctx* ctx() const { return ctx_; }
    int device() const { return device_; }
    /* gpu_handles.rs:72-90: is there a device to render on? */
    static bool self_test();
    void check(int rc, const char* what) const;

private:
    rt_ctx* ctx_ = nullptr;
    int device_ = 0;
};

/* ---- src/camera.rs */
using Vec3 = std::array<float, 3>;

struct Camera {   /* :13-34 */
    Vec3 eye{2.0f, 1.5f, 2.0f};
    Vec3 target{0.0f, 0.5f, 0.0f};
    Vec3 up{0.0f, 1.0f, 0.0f};
    float aspect = 1.0f;
    float constant = 1.0f;
};

/* winit VirtualKeyCode values the controller reacts to (camera.rs:56-81) */
enum class Key { W, A, S, D, Up, Down, Left, Right, Other };
Key key_from_name(const std::string& name);

class CameraController {   /* :36-112 */
public:
    explicit CameraController(float speed = 0.05f) : speed_(speed) {}   // CAMERA_SPEED, render_state.rs:31
    /* Command::KeyEvent: true when the key is one the controller owns */
    bool handle_camera_commands(Key key, bool pressed);
    /* f32 in cgmath's operation order (normalize = v * (1/|v|)) */
    void update_camera(Camera& camera) const;

private:
    float speed_;
    bool forward_ = false, backward_ = false, left_ = false, right_ = false;
};

/* ---- src/scenes.rs */
enum class VertexType { Split, Combined };
enum class TraverseType { Bsp, Bvh };

struct SceneDescriptor {   /* :20-44 */
    std::string name;
    std::string shader;                            // res/shaders/<file>
    VertexType vertex_type = VertexType::Split;
    std::optional<std::string> model;              // res/models/<file>
    std::optional<std::string> background_hdri;    // res/textures/<file>
    Camera camera;
    std::pair<uint32_t, uint32_t> res{512, 512};
    TraverseType traverse_type = TraverseType::Bsp;
    /* the rt_mode whose kernel restates the shader (mode_of_shader), the one a RenderState
     * renders; nullopt = no kernel does (w1e1.wgsl, the blank template) */
    std::optional<rt_mode> kernel_mode() const;
    /* kernel_mode() by family, each nullopt for every other scene -- */
    /* W1E6 or a family that walks a tree (RT_FAMILY_NEEDS_TREE) */
    std::optional<rt_mode> mode() const;
    /* mode(), or else the triangle sweep of the brute-force W5 scenes (RT_FAMILY_SWEEP) */
    std::optional<rt_mode> render_mode() const;
    /* an analytic W2 / W3 scene (RT_FAMILY_ANALYTIC) */
    std::optional<rt_mode> analytic_mode() const;
    /* W1 E2 .. W1 E5 (RT_FAMILY_WORKSHEET1 but W1E6) */
    std::optional<rt_mode> worksheet1_mode() const;
};

/* The row of the mode table (rt.h rt_mode_describe) whose shader file is `shader`, nullopt when
 * no kernel restates it: the lookup behind kernel_mode() and RenderState, part of this header's
 * interface for a host that wants the family and the flags with the mode.  Inline, so it needs
 * the C ABI library alone. */
inline std::optional<rt_mode_desc> mode_of_shader(const std::string& shader)
{
    rt_mode_desc d;
    for (int m = 0; m < RT_MODE_COUNT; m++)
        if (rt_mode_describe(m, &d) == RT_OK && shader == d.shader) return d;
    return std::nullopt;
}

std::vector<SceneDescriptor> get_scenes();            /* :46-488, the 44 scenes in order */
const SceneDescriptor& find_scene(const std::string& name);

/* ---- src/bindings/uniform.rs */
constexpr uint32_t MAX_SUBDIVISION = 10;
/* compute_jitters (:254-277): PCG32 Lcg64Xsh32::new(0, 0), rand's f64 gen_range */
std::vector<std::array<float, 2>> compute_jitters(double pixel_size, uint32_t subdivs);
/* selection2, use_texture and uv_scale default to the reference's (:152-156) */
rt_uniform make_uniform(const Camera& cam, uint32_t width, uint32_t height, uint32_t selection1 = 0,
                        uint32_t subdivision_level = 1, uint32_t iteration = 0, uint32_t selection2 = 0,
                        uint32_t use_texture = 0, std::array<float, 2> uv_scale = {1.0f, 1.0f});
/* deterministic stand-in for res/textures/grass.jpg (not redistributed): size x size
 * RGBA8 texels, the same integer arithmetic as core.synth_texture() */
std::vector<uint8_t> synth_texture(uint32_t size = 64);

/* PCG32 (XSH RR), as rand_pcg 0.3.1's Lcg64Xsh32 */
class Lcg64Xsh32 {
public:
    Lcg64Xsh32(uint64_t state, uint64_t stream);
    uint32_t next_u32();
    uint64_t next_u64();
    double gen_unit_f64();   // gen_range(0.0..1.0)

private:
    uint64_t state_, increment_;
};

/* ---- src/mesh.rs + src/data_structures (host builders behind the C ABI) */
class Mesh {
public:
    static Mesh load(const std::string& path);                   /* Mesh::from_obj */
    static Mesh synth_bunny(uint32_t ntris = 69451, uint32_t seed = 0x0B0B);
    Mesh(Mesh&& o) noexcept : m_(o.m_) { o.m_ = nullptr; }
    ~Mesh();
    rt_mesh_host* get() const { return m_; }
    uint32_t ntris() const;

private:
    explicit Mesh(rt_mesh_host* m) : m_(m) {}
    rt_mesh_host* m_;
};

/* n elements of device memory and their owner: rt_device_alloc .. rt_device_free.  Move-only; the
 * element type is the one the C ABI takes the buffer as.  Throws Error where the C ABI fails, but
 * for the free, whose status nobody could act on. */
template <class T>
class DeviceArray {
public:
    DeviceArray() = default;
    DeviceArray(const GpuHandles& gpu, size_t n, const char* what) : gpu_(&gpu), n_(n)
    {
        void* p = nullptr;
        gpu.check(rt_device_alloc(gpu.ctx(), n * sizeof(T), &p), what);
        p_ = static_cast<T*>(p);
    }
    DeviceArray(DeviceArray&& o) noexcept : gpu_(o.gpu_), p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DeviceArray& operator=(DeviceArray&& o) noexcept
    {
        if (this != &o) {
            reset();
            gpu_ = o.gpu_;
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DeviceArray() { reset(); }
    void reset()
    {
        if (p_) rt_device_free(gpu_->ctx(), p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }
    void zero(const char* what) { gpu_->check(rt_memset_device(gpu_->ctx(), p_, 0, n_ * sizeof(T)), what); }
    std::vector<T> download(const char* what) const
    {
        std::vector<T> out(n_);
        gpu_->check(rt_memcpy_to_host(gpu_->ctx(), out.data(), p_, n_ * sizeof(T)), what);
        return out;
    }

private:
    const GpuHandles* gpu_ = nullptr;
    T* p_ = nullptr;
    size_t n_ = 0;
};

/* ---- src/render_state.rs + src/lib.rs rendering_thread */
struct RenderOptions {
    std::string models_dir;                               // where scene models live
    std::optional<std::pair<uint32_t, uint32_t>> resolution;   // override SceneDescriptor.res
    bool bunny_standin = true;                            // bunny.obj is absent from the reference
    bool device_build = false;                            // build BSP / HLBVH on the GPU
    Vec3 environment{1.0f, 1.0f, 1.0f};                   // W9 escape radiance without a texture
};

/* Every device buffer of a RenderState is a DeviceArray member, so whatever throws -- the
 * constructor included -- leaves nothing allocated that the state does not still own.  A call that
 * enables something allocates and clears into locals and commits when all of it succeeded: one that
 * throws leaves the feature off.  A load_scene that throws leaves a state fit only for another
 * load_scene or the destructor. */
class RenderState {
public:
    RenderState(GpuHandles& gpu, const SceneDescriptor& scene, RenderOptions opts);
    ~RenderState();
    RenderState(const RenderState&) = delete;
    RenderState& operator=(const RenderState&) = delete;

    void load_scene(const SceneDescriptor& scene);   /* :314-334 (+ iteration reset, lib.rs:464-469) */
    void update();                                   /* :467-481 */
    void render(uint32_t spp = 1);                   /* :483-561, spp progressive iterations */
    bool step();                                     /* one pass of rendering_thread, lib.rs:331-363 */

    bool input_alt(Key key, bool pressed);           /* :462-465 */
    void update_camera_constant(float constant);     /* :591-593 */
    void set_samples(uint32_t samples, bool enabled);   /* Command::SetSamples, lib.rs:472-479 */
    void set_subdivision_level(uint32_t level);      /* uniform.rs:122-129 */
    void set_selection1(uint32_t shader);            /* Command::SetSphereMaterial, lib.rs:404-408 */
    void set_sphere_material(uint32_t shader) { set_selection1(shader); }
    void set_other_material(uint32_t shader);        /* Command::SetOtherMaterial, lib.rs:409-411 */
    void set_texture(uint32_t use_texture, std::array<float, 2> uv_scale);   /* Command::SetTexture, lib.rs:415-421 */
    /* texture0 of the W3 scenes, decoded by the caller (render_state.rs:179-189): RGBA8
     * texels, row 0 at v = 0; setup_rendering installs synth_texture() for them */
    void set_texture_image(const uint8_t* rgba8, uint32_t width, uint32_t height);
    /* the scene's background_hdri, decoded by the caller (render_state.rs:191-206):
     * RGBA8 equirectangular texels, or nullptr for the constant environment */
    void set_environment_map(const uint8_t* rgba8, uint32_t width, uint32_t height);
    void reset_iteration();
    /* Framebuffer tiling across the GPUs of a node: this state
     * renders only rank `rank`'s interleaved 8x8 tiles of every frame
     * (rt_render_tiles, into a packed accumulation kept across iterations) and
     * gathers all ranks' tiles into rank 0's frame over RCCL (rt_comm_init with
     * the communicator id rank 0 made, rt_gather_tiles).  Collective: every rank
     * calls it, then render()/step() in lockstep; frame()/hit_ids() are rank 0's.  When the
     * tile buffers cannot be allocated it throws and the state stays untiled; the communicator
     * rt_comm_init made stays in the context (rt_comm_destroy, or the context's end, removes it). */
    void set_tiling(uint32_t nranks, uint32_t rank, const uint8_t comm_id[RT_COMM_ID_BYTES]);

    /* The noise estimate of the path modes (rt.h "noise estimate"): from iteration 0 on, every
     * render keeps each pixel's running mean and variance of the iterations' luminance
     * (rt_set_noise_buffer; the buffer is reallocated by load_scene).  Throws for a mode that
     * writes no per-iteration records, after iteration 0, and on a tiled state: after set_tiling
     * (any rank count, 1 included) the renders index their outputs packed per tile, not as the
     * width x height buffer this allocates, and a summary across ranks is out of scope.  The
     * other noise calls throw on a tiled state too, and set_tiling throws once this is enabled. */
    void enable_noise();
    /* the relative standard error of every pixel after iteration() >= 2 iterations, H x W */
    std::vector<float> noise_map(float floor = 1e-3f) const;
    rt_noise_summary noise_summary(float threshold, float floor = 1e-3f) const;
    /* Render `batch` iterations at a time (the last batch clipped to max_samples) until at
     * most allow x pixels lie above the relative standard error `target` or max_samples
     * iterations are done.  Returns the iteration count; *summary (if given) receives the last
     * summary (zeroed when fewer than 2 iterations were rendered). */
    uint32_t render_until(float target, uint32_t max_samples, uint32_t batch = 16, double allow = 0.0,
                          float floor = 1e-3f, rt_noise_summary* summary = nullptr);

    /* Adaptive sampling (rt.h "adaptive sampling"): from iteration 0 on, every render traces
     * and folds only the pixels that have not converged -- a pixel (RT_ADAPT_PIXEL) or its 8x8
     * tile (RT_ADAPT_TILE) stops once it has min_samples iterations and its relative standard
     * error is at most target (rt_set_adaptive).  Enables the noise estimate if needed; the
     * count buffer is reallocated by load_scene.  As for the noise estimate: every adaptive
     * call throws on a tiled state, and set_tiling throws once this is enabled. */
    void enable_adaptive(float target, float floor = 1e-3f, uint32_t min_samples = 16, int vote = RT_ADAPT_TILE);
    std::vector<uint32_t> sample_counts() const;   /* the iterations folded into every pixel, H x W */
    rt_adaptive_summary adaptive_summary() const;
    /* Render `batch` iterations at a time (the last batch clipped to max_samples) until no pixel
     * is live any more or max_samples iterations are done.  Returns the iteration count;
     * *summary (if given) receives the last summary (zeroed when nothing was rendered). */
    uint32_t render_adaptive(uint32_t max_samples, uint32_t batch = 16, rt_adaptive_summary* summary = nullptr);

    /* The guide with objects (rt.h "denoise / Guide with objects").  Off (the default): the guide
     * of denoise, denoised_rgba8, temporal_step, temporal_frame and temporal_rgba8 is
     * rt_denoise_guide's, for which the W8 balls and the W9E2 / W9E3 holdout plane are background.
     * On: it is rt_denoise_guide_objects' with rt_guide_objects(mode()): those pixels get the
     * object's normal and depth, and a history; a mode without such objects is not changed.
     * Throws once temporal accumulation is enabled (a history's guide comes from one definition:
     * set it before enable_temporal); load_scene keeps it.  With a library that lacks the entry
     * points the first use throws RT_E_UNSUPPORTED. */
    void set_guide_objects(bool on);
    bool guide_objects() const { return guide_objects_; }

    /* The frame through the variance-guided a-trous filter (rt.h "denoise", rt_denoise): linear
     * RGBA32F, H x W x 4, alpha 1.  Needs enable_noise() and iteration() >= 2; under adaptive
     * sampling every pixel's variance uses its own sample count.  The accumulation, the ids and
     * the noise state are not changed.  Throws for a mode without a noise state and on a tiled
     * state (the filter needs every pixel's neighbours). */
    std::vector<float> denoise(uint32_t levels = 5, float sigma_l = 4.0f, float sigma_z = 1.0f) const;
    /* ... as the sRGB surface would hold it, H x W x 4 (rt_frame_rgba8_mode of denoise()) */
    std::vector<uint8_t> denoised_rgba8(uint32_t levels = 5, float sigma_l = 4.0f, float sigma_z = 1.0f) const;

    /* Temporal accumulation (rt.h "temporal accumulation"): frames that follow a moving camera.
     * temporal_step renders spp iterations of the sequence's own counter into a buffer of its
     * own, makes the guide, blends the frame with the history reprojected from the previous
     * camera (rt_temporal_accumulate), then update()s -- which moves the camera.  The progressive
     * accumulation, ids, iteration, noise and adaptive state are not touched; load_scene
     * reallocates.  Throws for a mode that writes no per-iteration records and on a tiled state
     * (reprojection needs every pixel's neighbours). */
    void enable_temporal(uint32_t max_history = 32, float normal_min = 0.9f, float plane_tol = 0.01f,
                         uint32_t min_len = 4);
    void disable_temporal();
    void temporal_step(uint32_t spp = 1);
    /* the latest integrated frame through rt_temporal_variance and rt_denoise_filter, H x W x 4 */
    std::vector<float> temporal_frame(uint32_t levels = 5, float sigma_l = 4.0f, float sigma_z = 1.0f) const;
    std::vector<uint8_t> temporal_rgba8(uint32_t levels = 5, float sigma_l = 4.0f, float sigma_z = 1.0f) const;
    /* the latest history: colour H x W x 4, luminance moments H x W x 2, length H x W */
    struct TemporalHistory {
        std::vector<float> color, moments;
        std::vector<uint32_t> length;
    };
    TemporalHistory temporal_history() const;
    /* the most recent temporal_step's own render -- its accumulation (the iterations folded into
     * zero, H x W x 4), its ids and the uniform it used -- for tests and tools */
    struct TemporalCurrent {
        std::vector<float> accum;
        std::vector<uint32_t> ids;
        rt_uniform uniform;
    };
    TemporalCurrent temporal_current() const;

    std::vector<float> frame() const;        /* linear RGBA32F accumulation, H x W x 4 */
    std::vector<uint32_t> hit_ids() const;   /* primary-hit triangle ids, H x W */
    /* the sRGB surface frame, H x W x 4 (rt_frame_rgba8_mode: W1E2 and W1E3 without the pow) */
    std::vector<uint8_t> frame_rgba8() const;

    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    uint32_t iteration() const { return iteration_; }
    const Camera& camera() const { return camera_; }
    const SceneDescriptor& scene() const { return scene_; }
    rt_mode mode() const { return (rt_mode)row_.mode; }   /* the rt_mode this state renders */
    rt_ray_counts last_counts() const;

private:
    void setup_rendering(const SceneDescriptor& scene);   /* :161-265 */
    void release();
    DeviceArray<float> denoise_device(uint32_t levels, float sigma_l, float sigma_z) const;
    DeviceArray<float> temporal_device(uint32_t levels, float sigma_l, float sigma_z) const;
    uint32_t guide_mask(const char* who) const;

    GpuHandles& gpu_;
    RenderOptions opts_;
    SceneDescriptor scene_;
    Camera camera_;
    CameraController controller_;
    rt_mode_desc row_{};   // the mode table's row of the scene's kernel_mode()
    rt_traverse trav_ = RT_TRAVERSE_BSP;
    uint32_t width_ = 0, height_ = 0;
    uint32_t iteration_ = 0, max_iterations_ = 2, subdivision_ = 1, selection1_ = 0;
    uint32_t selection2_ = 0, use_texture_ = 0;
    std::array<float, 2> uv_scale_{1.0f, 1.0f};
    bool progressive_ = true;
    DeviceArray<float> accum_;         // width x height RGBA32F
    DeviceArray<uint32_t> ids_;
    uint32_t nranks_ = 1, rank_ = 0;   // set_tiling
    bool tiled_ = false;
    DeviceArray<float> tile_accum_;    // this rank's packed tiles (rt_render_tiles)
    DeviceArray<uint32_t> tile_ids_;
    DeviceArray<rt_noise_state> noise_;   // enable_noise: width x height, registered with the context
    DeviceArray<uint32_t> counts_;     // enable_adaptive: width x height sample counts, registered too
    float ad_target_ = 0.0f, ad_floor_ = 1e-3f;
    uint32_t ad_min_ = 16;
    int ad_vote_ = RT_ADAPT_TILE;
    rt_uniform uniform_{};             // what update() last set
    // enable_temporal: the current frame, the guide's dz and two history sets {colour, moments, length, nz}
    struct TemporalSet {
        DeviceArray<float> color, mom, nz;
        DeviceArray<uint32_t> len;
    };
    bool guide_objects_ = false;       // set_guide_objects
    bool temporal_ = false;
    DeviceArray<float> tp_cur_, tp_dz_;
    DeviceArray<uint32_t> tp_ids_;
    TemporalSet tp_set_[2];
    int tp_latest_ = -1;               // the set of the latest frame; -1 before the first
    rt_uniform tp_uniform_{};          // the uniform that frame was rendered with
    uint32_t tp_k_ = 0, tp_max_history_ = 32, tp_min_len_ = 4;
    float tp_normal_min_ = 0.9f, tp_plane_tol_ = 0.01f;
};

}  // namespace raytracer
