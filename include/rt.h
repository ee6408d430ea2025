/*
 * rt.h -- C ABI of the MI355X-native hot path of cakarsubasi/02562_raytracer.
 *
 * The reference renders one frame per `RenderState::render()` call
 * (src/render_state.rs:483-561): a full-screen quad whose fragment shader
 * (`fs_main` of res/shaders/{w6e1,project,w7e3,w9e1,w1e6}.wgsl) traces one path
 * per pixel through the BSP (res/shaders/bsp.wgsl:10-81) or HLBVH
 * (res/shaders/bvh.wgsl:154-191).  This library replaces, behind plain C
 * pointers and sizes:
 *   - the wgpu device/queue wrapper          src/gpu_handles.rs:9-14, 72-92
 *   - the storage-buffer uploads             src/bindings/{storage_mesh,bsp_tree,bvh,uniform}.rs
 *   - the render pass + accumulation copy    src/render_state.rs:483-561
 *   - the fragment shader itself             res/shaders/<scene>.wgsl (HIP kernels for gfx950)
 * and exposes the host-side builders that feed it (the reference computes these
 * in Rust before upload):
 *   - Mesh::from_obj / Mesh::load            src/mesh.rs:78-202
 *   - BspTree::new + bsp_array + primitive_ids  src/data_structures/bsp_tree.rs:45,120,79
 *   - hlbvh::Bvh::new + flatten + triangles  src/data_structures/hlbvh.rs:36,195,237
 *
 * Conventions:
 *   - every function returns RT_OK (0) or a negative RT_E_* code; no exceptions
 *     cross the ABI; rt_last_error() gives a message for the last failure;
 *   - uploads copy from caller-owned host arrays (as wgpu create_buffer_init);
 *     the context owns all device memory it allocates;
 *   - a context is bound to one HIP device and is not thread-safe: use one
 *     context per GPU and per host thread (the reference uses its RenderState
 *     from the single "Render Thread", src/lib.rs:305-307);
 *   - output buffers passed to rt_render* are DEVICE pointers (HBM resident);
 *     their layout is documented per function.
 */
#ifndef RT02562_RT_H
#define RT02562_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------ */
#define RT_OK            0
#define RT_E_INVALID    (-1)  /* bad argument / malformed structure          */
#define RT_E_OOM        (-2)  /* device allocation failed (SurfaceError::OutOfMemory, src/lib.rs:345) */
#define RT_E_DEVICE     (-3)  /* HIP runtime error                           */
#define RT_E_NOT_READY  (-4)  /* render called before the needed upload      */
#define RT_E_IO         (-5)  /* file could not be read / parsed             */
#define RT_E_UNSUPPORTED (-6) /* mode/traversal combination not implemented  */

/* ---- plain data types (byte-compatible with the reference GPU structs) -- */

/* Material, 64 B: src/mesh.rs:12-20 (WGSL struct src/bindings/storage_mesh.rs:392-397) */
typedef struct rt_material {
    float diffuse[4];
    float ambient[4];
    float specular[4];
    uint32_t emissive;      /* MTL illum; == 1 marks an area light (storage_mesh.rs:322) */
    uint32_t _pad[3];
} rt_material;

/* HLBVH GpuNode, 32 B: src/data_structures/hlbvh.rs:508-515 */
typedef struct rt_gpu_node {
    float min[3];
    uint32_t offset_ptr;    /* leaf: first index into tri_ids; interior: right child */
    float max[3];
    uint32_t n_prims;       /* 0 = interior (left child is node+1) */
} rt_gpu_node;

/* Uniform block, 80 B: src/bindings/uniform.rs:6-34 */
typedef struct rt_uniform {
    float camera_pos[3];
    float camera_constant;
    float camera_look_at[3];
    float aspect_ratio;
    float camera_up[3];
    uint32_t selection1;     /* shader selector (0 = Lambertian) */
    uint32_t selection2;
    uint32_t subdivision_level;
    uint32_t use_texture;
    uint32_t iteration;      /* progressive frame index (overridden by first_iter) */
    float uv_scale[2];
    uint32_t resolution[2];  /* full-frame W, H (global pixel space) */
} rt_uniform;

/* Which scene shader the kernel restates (SceneDescriptor.shader, src/scenes.rs:19-29). */
typedef enum rt_mode {
    RT_MODE_W1E6    = 0,  /* res/shaders/w1e6.wgsl: analytic sphere/plane/triangle, no mesh  */
    RT_MODE_W6E1    = 1,  /* res/shaders/w6e1.wgsl: primary rays, directional light, split vertex layout */
    RT_MODE_PROJECT = 2,  /* res/shaders/project.wgsl: as W6E1, combined layout, ambient*0.1 */
    RT_MODE_W7E3    = 3,  /* res/shaders/w7e3.wgsl: area-light path tracer, progressive       */
    RT_MODE_W9E1    = 4,  /* res/shaders/w9e1.wgsl: dummy-light path tracer, environment escape */
    RT_MODE_W8E1    = 5,  /* res/shaders/w8e1.wgsl: Cornell box + mirror and glass balls, direct light */
    RT_MODE_W8E2    = 6,  /* res/shaders/w8e2.wgsl: as W8E1, path traced (Russian roulette, clamp 100) */
    RT_MODE_W8E3    = 7,  /* res/shaders/w8e3.wgsl: as W8E2, Beer-Lambert absorption in the glass ball */
    RT_MODE_W9E2    = 8,  /* res/shaders/w9e2.wgsl: W9E1 + holdout plane y=0 (AO any-hit), RGBE environment */
    RT_MODE_W6E2    = 9,  /* res/shaders/w6e2.wgsl: direct light from every area-light centre, subdiv^2 samples */
    RT_MODE_W7E1    = 10, /* res/shaders/w7e1.wgsl: as W6E2, progressive (TEA jitter), no max(., 0) */
    RT_MODE_W7E2    = 11, /* res/shaders/w7e2.wgsl: random area-light points, progressive */
    RT_MODE_W6E3    = 12, /* res/shaders/w6e3.wgsl: W6E2's box + mirror ball and glossy (Phong + refraction) ball */
    RT_MODE_W9E3    = 13, /* res/shaders/w9e3.wgsl: sun light, holdout plane (AO + sun rays), culled triangles */
    /* The brute-force worksheet-5 mesh scenes: no tree, every ray tests the triangles in
     * index-buffer order and takes the FIRST whose test accepts (intersect_scene_loop's
     * `has_hit || ...` short-circuits), not the closest.  RT_TRAVERSE_NONE only; they need
     * rt_upload_mesh and no BSP or BVH.  One frame per call (first_iter and spp are not read). */
    RT_MODE_W5E2    = 14, /* res/shaders/w5e2.wgsl: flat normals, directional light, one shadow sweep per hit */
    RT_MODE_W5E3    = 15, /* res/shaders/w5e3.wgsl: interpolated vertex normals, directional light, no shadow rays */
    RT_MODE_W5E4    = 16, /* res/shaders/w5e4.wgsl: material diffuse + ambient; no 1/subdiv^2 multiplier */
    RT_MODE_W5E5    = 17, /* res/shaders/w5e5.wgsl: every area-light centre, one shadow sweep per light and hit */
    /* The analytic worksheet-2 and worksheet-3 scenes: W1E6's triangle, sphere and plane with the
     * control panel's materials (uniforms.selection1: the sphere, selection2: the plane; 0 Lambertian,
     * 1 Phong, 2 mirror, 3 transmit, 4 glossy, 5 normal, 6 base colour -- a value the file's switch
     * does not know shades (0.7, 0, 0.7)), up to ten bounces, and from W3E1 on texture0 on the plane
     * (uniforms.use_texture, uv_scale; rt_set_texture).  intersect_scene takes the FIRST of triangle,
     * sphere, plane whose test accepts, not the closest.  RT_TRAVERSE_NONE only; no mesh, BSP or BVH.
     * One frame per call (first_iter and spp are not read).  DESIGN.md "Analytic worksheet scenes". */
    RT_MODE_W2E1    = 18, /* res/shaders/w2e1.wgsl: Lambertian everywhere (selections not read), black sphere */
    RT_MODE_W2E2    = 19, /* res/shaders/w2e2.wgsl: + selection1 / selection2, mirror (restarts at the hit point) */
    RT_MODE_W2E3    = 20, /* res/shaders/w2e3.wgsl: + transmit (ior 1.5), mirror offset by normal * 1e-5 */
    RT_MODE_W2E4    = 21, /* res/shaders/w2e4.wgsl: + Phong (specular 0.1, shininess 42), ior 1.4, diffuse x 0.9 */
    RT_MODE_W2E5    = 22, /* res/shaders/w2e5.wgsl: + glossy (Phong + transmit), transmit offset by w_t * 1e-5 */
    RT_MODE_W3E1    = 23, /* res/shaders/w3e1.wgsl: + texture0 on the plane, uv0 not wrapped (ClampToEdge) */
    RT_MODE_W3E2    = 24, /* res/shaders/w3e2.wgsl: uv0 % 1, fract(uv0 * uv_scale) */
    RT_MODE_W3E3    = 25, /* res/shaders/w3e3.wgsl: + subdivision_level^2 jittered samples */
    RT_MODE_W3E4    = 26, /* res/shaders/w3e4.wgsl: use_texture picks the sampler (1, 2 linear; 3 nearest), diffuse x 1 */
    /* The worksheet-1 scenes before W1E6, partial steps towards it: the uniforms alone (selections,
     * subdivision level and texture settings are not read).  W1E4 and W1E5 take the CLOSEST of triangle,
     * sphere, plane, as W1E6 does (each accepted test lowers tmax for the next).  W1E2 and W1E3 return their
     * colour without the pow(., 1.5) of every other shader: display them with rt_frame_rgba8_mode.
     * RT_TRAVERSE_NONE only; no mesh, BSP or BVH.  One frame per call (first_iter and spp are treated as
     * RT_MODE_W1E6 treats them).  W1E1, the blank template, has no mode.  DESIGN.md "Worksheet-1 scenes". */
    RT_MODE_W1E2    = 27, /* res/shaders/w1e2.wgsl: the quad scaled by 0.9 in (0.1, 0.3, 0.6), the clear colour (0, 0, 0) around it; no ray */
    RT_MODE_W1E3    = 28, /* res/shaders/w1e3.wgsl: the camera ray's direction as (q + 1) / 2; no aspect ratio, camera constant 1 */
    RT_MODE_W1E4    = 29, /* res/shaders/w1e4.wgsl: W1E3's ray, closest hit, the base colour alone (background on a miss) */
    RT_MODE_W1E5    = 30  /* res/shaders/w1e5.wgsl: as W1E4, the ray with the aspect ratio and the camera constant */
} rt_mode;
#define RT_MODE_COUNT 31   /* the rt_mode values are 0 .. RT_MODE_COUNT - 1 */

/* The kernel family of a mode: what a render of it needs uploaded and which traversals it takes. */
typedef enum rt_family {
    RT_FAMILY_WORKSHEET1 = 0,  /* the uniforms alone (rt_worksheet1.hip); RT_TRAVERSE_NONE only */
    RT_FAMILY_ANALYTIC   = 1,  /* three constant objects, materials, bounces, no mesh (rt_analytic.hip); NONE only */
    RT_FAMILY_SWEEP      = 2,  /* the mesh alone, every ray tests the triangle list (rt_sweep.hip); NONE only */
    RT_FAMILY_PRIMARY    = 3,  /* mesh + BSP or BVH: camera rays and a directional light, one frame per call */
    RT_FAMILY_DIRECT     = 4,  /* mesh + BSP or BVH: direct light from the area lights, folded inside the kernel */
    RT_FAMILY_PATH       = 5   /* mesh + BSP or BVH: every iteration's radiance is a record, folded in order; the
                                  noise estimate, adaptive sampling and the denoise filter follow these modes */
} rt_family;
#define RT_FAMILY_NEEDS_TREE(f) ((f) == RT_FAMILY_PRIMARY || (f) == RT_FAMILY_DIRECT || (f) == RT_FAMILY_PATH)
#define RT_FAMILY_NEEDS_MESH(f) ((f) == RT_FAMILY_SWEEP || RT_FAMILY_NEEDS_TREE(f))

/* rt_mode_desc.flags */
#define RT_MODEF_PROGRESSIVE    1u  /* first_iter and spp are read: a host advances its iteration by spp per render */
#define RT_MODEF_TEXTURE0       2u  /* samples texture0 (rt_set_texture) when uniforms.use_texture > 0 */
#define RT_MODEF_LINEAR_DISPLAY 4u  /* the shader returns its colour without the pow(., 1.5): rt_frame_rgba8_mode */
#define RT_MODEF_AREA_LIGHTS    8u  /* samples area lights: refused on a mesh with no emissive triangle */

/* One row of the mode table: everything the library and its hosts know about an rt_mode.
 * name and shader point to static strings ("W7E3", "w7e3.wgsl": the file under res/shaders). */
typedef struct rt_mode_desc {
    int32_t mode;        /* rt_mode */
    int32_t family;      /* rt_family */
    uint32_t flags;      /* RT_MODEF_* */
    uint32_t reserved;   /* 0 */
    const char* name;
    const char* shader;
} rt_mode_desc;

/* The row of `mode` into *out.  Needs no context.  RT_E_INVALID for a value that is no
 * rt_mode or a NULL out (*out is then left alone). */
int rt_mode_describe(int mode, rt_mode_desc* out);

/* SceneDescriptor.traverse_type, src/scenes.rs:13-17 */
typedef enum rt_traverse {
    RT_TRAVERSE_BSP  = 0,
    RT_TRAVERSE_BVH  = 1,
    RT_TRAVERSE_NONE = 2   /* the one traversal of the families that walk no tree (!RT_FAMILY_NEEDS_TREE); the
                              tree-walking families take BSP or BVH */
} rt_traverse;

/* A rectangle of the frame in GLOBAL pixel coordinates. */
typedef struct rt_tile {
    uint32_t x0, y0, w, h;
} rt_tile;

/* Interleaved 8x8-tile partition of the full frame for multi-GPU rendering
 * (SURVEY.md 8(e)): the tiles (ceil(W/8) x ceil(H/8)) are taken in sequence
 * s = ty * tiles_x + (tx - (ty & 7)) mod tiles_x -- row-major, each row rotated
 * by its index mod 8 (not rotated when tiles_x < 8) -- and sequence position s
 * is owned by rank s % nranks (diagonal stripes: on a rotated frame, when
 * nranks divides 8 and tiles_x, rank r owns tx = r + ty mod nranks; a frame
 * under 8 tiles wide is not rotated, and rank r then owns the whole columns
 * tx = r mod nranks).
 * Global pixel coordinates keep PRNG seeds, and therefore images, identical
 * for every nranks. */
typedef struct rt_tileset {
    uint32_t rank;
    uint32_t nranks;
} rt_tileset;

#define RT_TILE_DIM 8u    /* tile edge in pixels: one wave64 = one 8x8 tile */

/* Per-launch counters.  primary/shadow/bounce are always filled; the traversal
 * detail counters are filled only when RT_OPT_DETAIL_COUNTERS is enabled (a
 * separate, slower kernel instantiation used to price algorithmic bytes). */
typedef struct rt_ray_counts {
    uint64_t samples;        /* pixel-samples traced                       */
    uint64_t primary;        /* camera rays                                */
    uint64_t shadow;         /* shadow (visibility) rays                   */
    uint64_t bounce;         /* indirect closest-hit rays                  */
    uint64_t node_interior;  /* BSP interior node visits                   */
    uint64_t node_leaf;      /* BSP leaf visits                            */
    uint64_t bvh_pops;       /* BVH node pops                              */
    uint64_t ids_read;       /* treeIds / bvh_triangles reads              */
    uint64_t tri_tests;      /* ray-triangle tests                         */
    uint64_t tri_accepts;    /* accepted (closer) hits                     */
    /* SIMD-efficiency diagnostics (detail instantiation only), per wave trip
     * of the traversal loop: */
    uint64_t trips;          /* traversal loop trips (sum over waves)      */
    uint64_t lane_steps;     /* lanes that advanced a ray in those trips    */
    uint64_t leaf_lane_steps;/* ... of which were inside a leaf (triangle)  */
    uint64_t node_trips;     /* trips in which some lane walked nodes       */
    uint64_t leaf_trips;     /* trips in which some lane tested a triangle  */
    uint64_t exact_tests;    /* triangle tests that needed exact division   */
    uint64_t exact_nodes;    /* node decisions that needed exact division   */
    /* path kernels, per wave: shading passes, lanes shaded, and wave cycles
     * (s_memtime) spent in the traversal and in the shading/refill phases */
    uint64_t shade_passes;
    uint64_t shade_lanes;
    uint64_t trav_cycles;
    uint64_t shade_cycles;
    uint64_t memwait_cycles; /* BSP trips: wave cycles from load issue to data */
    uint64_t subtree_culls;  /* BSP walking trips that skipped their node's subtree (content box missed) */
} rt_ray_counts;

/* ---- options (rt_set_option) ------------------------------------------- */
#define RT_OPT_DETAIL_COUNTERS 1  /* 0/1: use the counting kernel instantiation    */
#define RT_OPT_WAVES_PER_CU    2  /* persistent grid size: waves per CU (default 32; capped by LDS) */
#define RT_OPT_SHADE_THRESHOLD 3  /* path kernels: shade once <= N of 64 lanes still trace; 0 or 64 = all lanes finish their rays first (lockstep); -1 = the default: 24 for W7E3 on the BSP walk, 4 for the BVH walk, and for the other modes on the BSP walk a per-wave choice from the share of its tracing lanes inside a leaf (the higher when >= 1/2): 20 or 32 with certified culling (24 or 32 when the silhouette kernel runs), 8 or 24 otherwise; 0x10000 | hi << 8 | lo sets that choice's two thresholds */
#define RT_OPT_SAMPLE_CHUNK    4  /* W7E3/W9E1: progressive iterations per work unit (default 1) */
#define RT_OPT_SAMPLE_BUDGET_MB 5 /* W7E3/W9E1: device scratch for per-sample results, MiB (default 16384);
                                     a render whose spp x pixels x 16 B exceed it runs in several passes */
#define RT_OPT_KERNEL_TIMING   7  /* 0/1: record HIP events around every traversal-kernel launch */
/* option 8 is retired (trip-half postponement: slower on every BASELINE workload, and its
   per-trip test cost 1.7-4.4 % even when off, profiles/r02/sweep_KH_c5.txt, ab_nokh.txt) */
#define RT_OPT_UNIT_ORDER      6  /* W7E3/W9E1 work-unit order: 0 chunk-major, 1 pixel-major (default) */
#define RT_OPT_ASYNC_FOLD     10  /* 0 (default) / 1: pipelined frames.  The path tracers' progressive fold (the
                                     last step of rt_render / rt_render_tiles) runs on a second, context-owned
                                     stream, and so do the calls that consume its outputs (rt_unpack_tiles,
                                     rt_gather_tiles; rt_frame_rgba8 joins that stream and runs on the
                                     context stream); the per-sample scratch is double-buffered.
                                     The next render's traversal kernel then overlaps this frame's fold and
                                     gather.  rt_synchronize, the memcpy/memset calls and every other entry point
                                     wait for that stream first; a caller reading the outputs through its own
                                     stream synchronizes the device (or calls rt_synchronize) first. */
#define RT_OPT_BSP_CULL        9  /* subtree culling in the BSP walk: a subtree whose content
                                     box (the union of its triangles' bounding boxes), grown by a margin, the ray
                                     interval misses is skipped, and the walk's decisions use the interval clipped to
                                     that box.  One of RT_BSP_CULL_*: */
#define RT_BSP_CULL_OFF        0  /* every node of bsp.wgsl's walk is visited: the reference's walk and tested-
                                     triangle sequence, by construction */
#define RT_BSP_CULL_CERTIFIED  1  /* the margin is a proven bound on how far an f32 accept of
                                     intersect_triangle (w7e3.wgsl:286-332) can lie from its triangle's box, from the
                                     subtree's largest edge, its box of normals and, for rays that start at the
                                     uniforms' camera eye, its per-eye plane distance: every hit (triangle, distance,
                                     barycentrics) is bit-identical to RT_BSP_CULL_OFF for every ray; only hitless
                                     work is skipped */
#define RT_BSP_CULL_FAST       2  /* the margin is 2^-10 of the scene's / the ray origin's coordinate magnitude: not
                                     a proven bound.  A ray within ~1e-5 rad of a large triangle's plane, where the
                                     f32 test's hit point can sit off the triangle by more than the margin, can get
                                     a different hit (measured: 2 of 400,000 deliberately grazing rays on a random
                                     soup, none in any rendered frame) */
#define RT_BSP_CULL_SILHOUETTE 3  /* the certified margin, exact as RT_BSP_CULL_CERTIFIED, with a tighter bound for
                                     camera rays: each subtree's two triangles nearest the eye's plane-distance
                                     floor (its silhouette) are bounded per ray by their own normals, the rest by
                                     their camera term.  Fewer trips for far, many-object views (config 4: +15 %),
                                     more arithmetic per trip (config 3: -4 %, config 5: -3 %).  The W9E1
                                     path kernel and rt_trace_batch use it; other kernels run the certified form */
#define RT_BSP_CULL_AUTO       4  /* (default) exact as RT_BSP_CULL_CERTIFIED: the W9E1 BSP renders time the
                                     certified and the silhouette kernels on four of their own launches (certified,
                                     silhouette, certified, silhouette; each at least 2^20 samples: a big render
                                     splits its first iterations, up to an eighth of it or 2^26 samples per
                                     launch, 1-spp frames give one launch each), with no extra
                                     work and no host wait (the events are read at a later render; the certified
                                     kernel runs until then), and run the faster from then on (the silhouette
                                     kernel must be 5 % faster to be chosen), until the BSP or this option changes
                                     or the eye's reach (farthest distance to the scene box) leaves [1/2, 2] of the
                                     reach the probe ran at.  rt_bsp_cull_in_use reports the choice */
#define RT_OPT_EMPTY_PIXELS   11  /* 1 (default) / 0: W9E1 on the BSP walk, with the constant environment (no
                                     rt_set_environment_map), a finite eye, no jitter table and no ray capture,
                                     casts no camera ray for a pixel that PROVABLY misses the mesh at every
                                     iteration: per camera, one bit per pixel says that intersect_triangle can accept
                                     no triangle for any direction of the pixel's footprint (grown by a whole pixel),
                                     by the certified margin of RT_BSP_CULL_CERTIFIED bounded over that footprint
                                     (DESIGN.md section 4 "Empty pixels").  Such a pixel's iterations all store
                                     vec3(0) + env * vec3(1) with primary id none; the fold and the noise estimate
                                     take that constant instead of reading records, so accum, ids, the noise state
                                     and rt_ray_counts (primary = the rays the reference's shader casts) are the
                                     same bits as with 0.  The mask is built once the iterations rendered with an
                                     unchanged camera, the call's own included, reach 96 (a 256-spp call builds it
                                     at once, a camera that moves every 1-spp frame never does), and dropped when
                                     the uniforms, the mesh or the BSP change.  rt_empty_pixels_in_use reports it */
#define RT_OPT_PIXEL_DEPTH    12  /* 1 (default) / 0: whenever a render uses the mask of RT_OPT_EMPTY_PIXELS, the camera
                                     rays of its pixels start their BSP walk on the pixel's certified depth range
                                     instead of [1e-4, tmax]: with the mask, and by the same margin, the build folds
                                     for every pixel a near and a far such that every distance intersect_triangle can
                                     accept for any camera ray of the pixel lies strictly between them.  The walk on
                                     that interval visits a subsequence of the reference walk's leaves and returns its
                                     hit (DESIGN.md section 4 "Pixel depth ranges"): accum, ids, the noise state and
                                     rt_ray_counts are the same bits as with 0.  Bounce rays are untouched, and with
                                     RT_BSP_CULL_OFF the walk keeps the reference's interval */
#define RT_OPT_DENOISE_LDS_STEP 13 /* the largest step 2^i at which a level of the denoise filter stages its tile and
                                     halo in LDS; larger steps load every tap from global memory.  0 (never), 1, 2,
                                     4 or 8 (default 4: DESIGN.md section 4 "Denoise"); every form gives the same bits */
#define RT_OPT_DENOISE_LATTICE_STEP 14 /* the smallest step from which a level runs the lattice form instead (a block per
                                     16 x 16 lattice of stride 2^i, a 20 x 20 LDS tile at every step): 0 (never, the
                                     default: it measured slower), 2, 4, 8 or 16; it takes precedence over the above */
#define RT_OPT_TEMPORAL_VAR_LDS 15 /* 1 (default) / 0: rt_temporal_variance stages its block's 22 x 22 tile of moments and
                                     guide in LDS, or loads every neighbour from global memory (the LDS form measured
                                     2.2 x faster: DESIGN.md section 4 "Temporal accumulation"); the same bits */

/* ---- device / context (replaces src/gpu_handles.rs) -------------------- */

typedef struct rt_ctx rt_ctx;   /* one HIP device + stream + the device-resident scene */

/* Number of HIP devices (~ gpu_handles::self_test, src/gpu_handles.rs:72-92). */
int rt_device_count(int* count);

/* Create a context on HIP device `device` (~ GPUHandles::new / RenderState::new
 * device part, src/render_state.rs:66-106).  Creates its own non-blocking stream. */
int rt_create(int device, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);

/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)
 * instead of the context's own stream; NULL restores the own stream. */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);
void* rt_get_stream(rt_ctx* ctx);
int rt_synchronize(rt_ctx* ctx);

int rt_set_option(rt_ctx* ctx, int option, int64_t value);

/* The culling mode the W9E1 BSP path kernel (and the query and batch kernels) run now
 * (RT_BSP_CULL_*): the option's value, except that RT_BSP_CULL_SILHOUETTE without the
 * eye's camera terms runs CERTIFIED and RT_BSP_CULL_AUTO runs its probe's choice
 * (CERTIFIED or SILHOUETTE; CERTIFIED until a probe has decided for the current BSP).
 * Kernels without a silhouette form (the other modes, W9E1's transparent shader) run
 * CERTIFIED under SILHOUETTE and AUTO.  probe_ms (2 floats, or NULL): the probe's best
 * certified and silhouette times in milliseconds per 2^20 samples, 0 until it has decided.
 * probes (2 uint32, or NULL): the probes this context has started and their launches. */
int rt_bsp_cull_in_use(rt_ctx* ctx, int* mode, float* probe_ms, uint32_t* probes);

/* RT_OPT_EMPTY_PIXELS: the mask the most recent render used.  pixels_flagged (or NULL):
 * the full-frame pixels flagged empty, 0 when that render used no mask (the option off,
 * a mode or setting the option does not cover, too few iterations yet).  build_ms (or
 * NULL): what the last mask build took on the device in milliseconds (0 until one ran). */
int rt_empty_pixels_in_use(rt_ctx* ctx, uint64_t* pixels_flagged, float* build_ms);

/* The same mask on the host, without a device: bit y * width + x of mask_words
 * (ceil(width * height / 32) words) is set when pixel (x, y) of the uniforms' camera is
 * empty for the mesh (nverts x float4 positions, ntris x (v0, v1, v2, material)).  The
 * device mask of a context with this mesh and these uniforms is the same bits.
 * *flagged (or NULL): the set bits.  A degenerate camera, a non-finite eye or
 * subdivision_level > 1 flag nothing. */
int rt_empty_mask_host(const float* pos_vec4, uint32_t nverts, const uint32_t* idx_vec4, uint32_t ntris,
                       const rt_uniform* u, uint32_t* mask_words, uint64_t* flagged);
/* The device mask of the most recent render into mask_words (host), all zero when it used
 * none (synchronizes). */
int rt_download_empty_mask(rt_ctx* ctx, uint32_t* mask_words, uint64_t nwords);
/* RT_OPT_PIXEL_DEPTH on the host, without a device (the sibling of rt_empty_mask_host, same
 * inputs): near_out / far_out [y * width + x] bound every distance that intersect_triangle
 * can accept for a camera ray of pixel (x, y), strictly.  A pixel rt_empty_mask_host flags
 * has near = +inf and far = 0; a pixel a non-finite triangle marks, and every pixel where
 * that entry point flags nothing for want of a mask, has near = 0 and far = +inf.  The
 * device arrays of a context with this mesh and these uniforms are the same bits. */
int rt_pixel_depth_host(const float* pos_vec4, uint32_t nverts, const uint32_t* idx_vec4, uint32_t ntris,
                        const rt_uniform* u, float* near_out, float* far_out);
/* The device ranges the most recent render's camera rays started on, npix = width * height
 * floats each (synchronizes); *in_use (or NULL) = 0 and near = 0, far = +inf when it used none. */
int rt_last_pixel_depth(rt_ctx* ctx, float* near_out, float* far_out, uint64_t npix, int* in_use);
/* Message describing the last failure on this context (or the last
 * context-less failure when ctx == NULL).  Never NULL. */
const char* rt_last_error(const rt_ctx* ctx);

/* Device memory for frame buffers (the RenderSource/RenderDestination
 * textures of src/bindings/texture.rs:285-407 become plain HBM arrays).
 * Copies synchronize the context stream; memset is asynchronous on it. */
int rt_device_alloc(rt_ctx* ctx, size_t bytes, void** dptr);
int rt_device_free(rt_ctx* ctx, void* dptr);
int rt_memcpy_to_host(rt_ctx* ctx, void* dst, const void* src_dev, size_t bytes);
int rt_memcpy_to_device(rt_ctx* ctx, void* dst_dev, const void* src, size_t bytes);
int rt_memset_device(rt_ctx* ctx, void* dst_dev, int value, size_t bytes);

/* HIP-event timer on the context stream (RenderStats, src/tools.rs:4-61,
 * times render() on the host; this times the device work). */
int rt_timer_start(rt_ctx* ctx);
int rt_timer_stop(rt_ctx* ctx, float* ms);   /* synchronizes */

/* Per-launch timing of the traversal kernels (k_path / k_primary / k_sweep / k_analytic / k_w1),
 * enabled by RT_OPT_KERNEL_TIMING: HIP events around every such launch on the
 * context stream.  rt_kernel_time synchronizes and returns the summed
 * duration and the number of launches since the last reset (reset != 0
 * clears them).  At most 4096 launches are kept between resets. */
int rt_kernel_time(rt_ctx* ctx, int reset, double* total_ms, uint32_t* launches);

/* The same for the frame's assembly (RT_OPT_KERNEL_TIMING): HIP events on the
 * output stream around the RCCL transfers of rt_gather_tiles (rank 0: the copy of
 * its own tiles and every peer's receive; another rank: its send) and around the
 * unpack kernel (rt_gather_tiles on rank 0, rt_unpack_tiles).  Synchronizes and
 * returns the summed times and the number of calls since the last reset (at
 * most 4096 calls are kept between resets).  For a multi-GPU host's per-rank
 * diagnostics (bench.py's N>1 line). */
int rt_gather_time(rt_ctx* ctx, int reset, double* transfer_ms, double* unpack_ms, uint32_t* calls);

/* ---- uploads (replace the src/bindings/ create_buffer_init calls) ------------- */

/* Mesh + materials + light list (src/bindings/storage_mesh.rs:13-26, 82-110,
 * 201-236, 297-332).  pos_vec4 / nrm_vec4: nverts x float4 (w ignored);
 * nrm_vec4 may be NULL (zero normals, as mesh.rs:165-171).  idx_vec4u: ntris x
 * (v0, v1, v2, material).  light_idx[0] must be the UINT32_MAX sentinel
 * (storage_mesh.rs:325-326); light_idx may be NULL to derive the list from
 * materials[].emissive == 1. */
int rt_upload_mesh(rt_ctx* ctx,
                   const float* pos_vec4, const float* nrm_vec4, uint32_t nverts,
                   const uint32_t* idx_vec4u, uint32_t ntris,
                   const rt_material* mats, uint32_t nmats,
                   const uint32_t* light_idx, uint32_t nlight);

/* Flattened BSP (src/bindings/bsp_tree.rs:167-203): aabb = BboxGpu (min.xyz,
 * pad, max.xyz, pad); tree_vec4u = nnodes x (axis|count<<2, first_id, left,
 * right) with nnodes == 2^(max_depth+1)-1; planes = nnodes floats; ids = nids
 * triangle indices.  Requires a prior rt_upload_mesh (triangles are repacked
 * in treeIds order on upload). */
int rt_upload_bsp(rt_ctx* ctx, const float aabb[8],
                  const uint32_t* tree_vec4u, const float* planes, uint32_t nnodes,
                  const uint32_t* ids, uint32_t nids, uint32_t max_depth);

/* Flattened HLBVH (src/bindings/bvh.rs:75-93). Requires a prior rt_upload_mesh. */
int rt_upload_bvh(rt_ctx* ctx, const rt_gpu_node* nodes, uint32_t nnodes,
                  const uint32_t* tri_ids, uint32_t nids);

/* Uniforms + jitter table (src/bindings/uniform.rs:163-176).  jitter holds
 * subdivision_level^2 float2 offsets (may be NULL when subdivision_level == 1:
 * compute_jitters returns (0,0), uniform.rs:261-263).  RT_E_INVALID for a zero
 * resolution or one above 65535 in either axis (the path kernel packs a pixel's
 * coordinates into one 32-bit register). */
int rt_set_uniforms(rt_ctx* ctx, const rt_uniform* u, const float* jitter);

/* ---- acceleration-structure construction on the GPU ---- */

/* Per-phase times of a device build, the reference's BvhConstructionTime
 * split (src/data_structures/bvh_util.rs:6-13, src/bin/bvh_project.rs). */
typedef struct rt_bvh_build_times {
    double morton_codes_ms, radix_sort_ms, treelet_init_ms, treelet_build_ms;
    double upper_tree_ms;        /* device-to-host of the treelet roots + host collapse + upload */
    double upper_tree_host_ms;   /* of which the host collapse                                    */
    double flattening_ms;        /* DFS offsets, GpuNode array, filler                            */
    double total_ms;             /* wall clock of the whole call                                  */
    uint32_t treelets, nodes;
} rt_bvh_build_times;

/* hlbvh::Bvh::new(mesh, max_prims) + flatten() + triangles()
 * (src/data_structures/hlbvh.rs:36-239) on the device from the context's
 * uploaded mesh: the same arrays as rt_bvh_build (equal Morton codes in
 * primitive-index order), installed as the context's BVH as rt_upload_bvh
 * would.  times may be NULL.  Synchronizes the context stream. */
int rt_build_bvh_device(rt_ctx* ctx, uint32_t max_prims, rt_bvh_build_times* times);

/* Per-phase times of a device BSP build (src/bin/bvh_project.rs
 * BspConstructionTime: subdivision, flattening). */
typedef struct rt_bsp_build_times {
    double subdivision_ms;   /* the level-by-level subdivide_node of every depth       */
    double flattening_ms;    /* leaf first-ids in DFS order + primitive_ids            */
    double total_ms;         /* wall clock of the whole call                           */
    uint32_t levels, leaves, nids;
} rt_bsp_build_times;

/* BspTree::new(mesh.bboxes(), max_depth, max_leaf) + bsp_array() +
 * primitive_ids() (src/data_structures/bsp_tree.rs:45-189, 195-323) on the
 * device from the context's uploaded mesh: the same arrays as rt_bsp_build,
 * installed as the context's BSP as rt_upload_bsp would.  Subdivision runs
 * one depth level at a time over all nodes of that level.  times may be NULL.
 * Synchronizes the context stream. */
int rt_build_bsp_device(rt_ctx* ctx, uint32_t max_depth, uint32_t max_leaf, rt_bsp_build_times* times);

/* Copy the context's BSP in the reference layout (bsp_array vec4u, planes,
 * primitive_ids, BboxGpu aabb[8]) to host arrays; sizes stored in nnodes/nids
 * (pass NULL arrays to query them). */
int rt_download_bsp(rt_ctx* ctx, uint32_t* tree, float* planes, uint32_t cap_nodes, uint32_t* ids,
                    uint32_t cap_ids, float aabb[8], uint32_t* nnodes, uint32_t* nids);

/* Diagnostics (no reference counterpart; tests/test_gpu_cert_data.py): copy the
 * BSP walk's 96-B treelets (slot 0 unused, then one per 1-based node M:
 * content box, nodes M, 2M, 2M+1, 4M..4M+3, and the certified culling's data
 * -- F bf16 | camera term G f16 << 16, normal-box centre and radius as f16;
 * rt_layout.hip k_bsp_repack) to dst, (nnodes + 1) * 96 bytes, followed by
 * RT_BSP_CULL_SILHOUETTE's node data ((nnodes + 1) * 16 bytes: the two excluded
 * triangles' n* / E^2 as f16 triples, the rest's camera term G_x f16; zero when
 * not computed), after bringing the camera terms up to date for the uniforms'
 * eye (certified culling).  The size is stored in *bytes (pass dst NULL to
 * query it). */
int rt_download_bsp_treelets(rt_ctx* ctx, void* dst, uint64_t cap_bytes, uint64_t* bytes);

/* Copy the context's BVH in the reference layout (GpuNode array, bvh_triangles)
 * to host arrays of capacity cap_nodes / cap_ids; the sizes are stored in
 * nnodes / nids (pass NULL arrays to query them). */
int rt_download_bvh(rt_ctx* ctx, rt_gpu_node* nodes, uint32_t cap_nodes, uint32_t* tri_ids, uint32_t cap_ids,
                    uint32_t* nnodes, uint32_t* nids);

/* Environment radiance returned on escape by RT_MODE_W9E1 (stands in for the
 * equirectangular hdri0 texture, res/shaders/w9e1.wgsl:232-241). Default (1,1,1). */
int rt_set_environment(rt_ctx* ctx, const float rgb[3]);

/* The hdri0 equirectangular background of the W9E1 scenes (src/scenes.rs
 * background_hdri; src/bindings/texture.rs: Rgba8Unorm, image.to_rgba8()):
 * width x height RGBA8 texels, row 0 at the top (v = 0).  Sampled by
 * environment_map (w9e1.wgsl:232-239) as include/rt_detmath.h pins it.
 * NULL removes it (the constant of rt_set_environment applies again). */
int rt_set_environment_map(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* texture0 of the W3 scenes (the reference builds res/textures/grass.jpg into every
 * RenderState: Rgba8Unorm, image.to_rgba8(), one mip level, ClampToEdge,
 * src/bindings/texture.rs:98-141): width x height RGBA8 texels, row 0 at v = 0,
 * copied to the device.  Sampled by texture_sample (w3e1.wgsl:189-193 ..
 * w3e4.wgsl:196-215) as include/rt_detmath.h rt_det_tex_sample pins it.  NULL
 * removes it; RT_E_INVALID for a zero size with data.  RT_MODE_W3E1..W3E4
 * rendered with uniforms.use_texture > 0 and no texture give RT_E_NOT_READY;
 * the W2 modes never read it. */
int rt_set_texture(rt_ctx* ctx, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* ---- render (replaces RenderState::render, src/render_state.rs:483-561) -- */

/* Trace `spp` progressive iterations first_iter .. first_iter+spp-1 for every
 * pixel of `region` (global pixel coordinates inside uniforms.resolution).
 * W7E3/W9E1 split the iterations of a pixel into work units of
 * RT_OPT_SAMPLE_CHUNK iterations that run in parallel; each unit writes its
 * per-iteration radiance to device scratch, and a fold kernel then applies the
 * reference's progressive average in iteration order (bit-identical to
 * `spp` sequential render() calls).
 *   accum_rgba32f: DEVICE, region.w*region.h float4, row-major over the region,
 *     in/out: holds the accumulation of iterations < first_iter (read when
 *     first_iter > 0; the RenderDestination texture, render_state.rs:541-555),
 *     and receives max(vec4(accum,1),0) (w7e3.wgsl:261-271).  For W1E6/W6E1/
 *     PROJECT, W5E2..W5E5, W2E1..W3E4 and W1E2..W1E5 it receives the linear
 *     per-frame result (before pow(.,1.5); W1E2 and W1E3 have none), alpha 1.
 *   primary_hit_ids: DEVICE or NULL, region.w*region.h u32: triangle index of
 *     the primary hit of the LAST traced iteration, UINT32_MAX on miss.  The
 *     analytic modes (W1E6, W2E1..W3E4) store the object the camera ray of the
 *     last sample accepted: 0 triangle, 1 sphere, 2 plane.  W1E4 and W1E5
 *     store the closest object as W1E6 does; W1E2 and W1E3 store UINT32_MAX.
 *   counts: host pointer or NULL; when non-NULL the call synchronizes and
 *     stores this launch's counters. */
int rt_render(rt_ctx* ctx, rt_mode mode, rt_traverse trav, const rt_tile* region,
              uint32_t first_iter, uint32_t spp,
              float* accum_rgba32f, uint32_t* primary_hit_ids,
              rt_ray_counts* counts);

/* Same, over the 8x8 tiles owned by `ts` (multi-GPU framebuffer tiling).
 * Outputs are PACKED: local tile l (the tile at sequence position
 * s = l*nranks + rank, rt_tileset above) occupies pixels [l*64, l*64+64),
 * row-major inside the tile: slot l*64 + (y & 7)*8 + (x & 7) holds pixel (x, y).
 * Buffers hold rt_tileset_local_tiles() * 64 px.  Padding: a slot that holds no
 * pixel of the frame -- the lanes of an edge tile past the right or bottom
 * edge, and every slot of a local tile whose sequence position is past the
 * last tile (ranks own ceil(ntiles / nranks) tiles each) -- is neither read
 * nor written by this call and keeps what it held; rt_gather_tiles transfers
 * it as it is and rt_unpack_tiles drops it. */
int rt_render_tiles(rt_ctx* ctx, rt_mode mode, rt_traverse trav, const rt_tileset* ts,
                    uint32_t first_iter, uint32_t spp,
                    float* accum_rgba32f, uint32_t* primary_hit_ids,
                    rt_ray_counts* counts);

/* Number of local tiles rank `rank` owns for a W x H frame (equal for all ranks
 * rounded up, so packed buffers have one size: ceil(ntiles / nranks)). */
uint32_t rt_tileset_local_tiles(uint32_t width, uint32_t height, uint32_t nranks);

/* The displayed frame of fs_main (w7e3.wgsl:261-271): saturate(pow(accum, 1.5))
 * as the sRGB surface stores it (render_state.rs:108-115), 8-bit RGBA, for
 * npix pixels; device pointers, asynchronous on the context stream.  The
 * pow and the sRGB rounding are pinned here (the display path is outside
 * the parity contract). */
int rt_frame_rgba8(rt_ctx* ctx, const float* accum_rgba32f, uint32_t npix, uint8_t* frame_rgba8);

/* The displayed frame of `mode`'s fs_main.  w1e2.wgsl and w1e3.wgsl return their colour
 * as it is, without the pow: for RT_MODE_W1E2 and RT_MODE_W1E3 the 8-bit code is the sRGB
 * code of saturate(accum), by the same thresholds and rounding as rt_frame_rgba8.  For
 * every other rt_mode the output is rt_frame_rgba8's, byte for byte.  NULL and empty
 * arguments behave as rt_frame_rgba8's do; RT_E_INVALID for a value that is no rt_mode. */
int rt_frame_rgba8_mode(rt_ctx* ctx, rt_mode mode, const float* accum_rgba32f, uint32_t npix, uint8_t* frame_rgba8);

/* Scatter gathered packed buffers (nranks x local_tiles x 64 px, rank-major as
 * a gather to the root produces them) into a row-major W x H frame, on the context's
 * stream.  Either pair of pointers may be NULL. */
int rt_unpack_tiles(rt_ctx* ctx, uint32_t width, uint32_t height, uint32_t nranks,
                    const float* packed_accum, const uint32_t* packed_ids,
                    float* frame_accum, uint32_t* frame_ids);

/* ---- noise estimate of the path modes (DESIGN.md section 4 "Noise estimate") ----
 * The seven path modes (W7E3, W9E1, W8E1..W8E3, W9E2, W9E3) write every iteration's
 * radiance as a record before the fold averages them.  With a noise buffer set, their
 * renders also keep, per output slot, the running mean and the sum of squared
 * deviations (Welford) of the iterations' luminance -- no reference counterpart: the
 * reference's sample count is a number the user guesses.  Pinned f32 arithmetic (no
 * contraction, correctly rounded / and sqrt).  For the record x of iteration `it`
 * (global index), in iteration order:
 *     y = (0.2126f*x.x + 0.7152f*x.y) + 0.0722f*x.z     the raw result, not the max(., 0) average
 *     n = (float)(it + 1)
 *     d = y - mean;  mean = mean + d / n;  m2 = m2 + d * (y - mean)
 * A pass with first_iter == 0 starts from {0, 0}; one with first_iter > 0 continues the
 * stored state (the caller keeps the iterations contiguous, as for accum).  Non-finite
 * samples propagate.  The state does not depend on how a render is split into launches,
 * passes, work units or tiles.  The relative standard error of the mean after n >= 2
 * iterations, with nf = (float)n and a floor > 0, is
 *     rel = sqrtf((m2 < 0 ? 0 : m2) / (nf * (nf - 1.0f))) / max(|mean|, floor)
 * A state with a non-finite field is "non-finite": its rel is the quiet NaN 0x7FC00000.
 * Alignment: the kernels move a state as one 8-byte word and a record as one 16-byte word,
 * so every state_dev pointer below must be 8-byte aligned and samples_rgba_dev 16-byte
 * aligned (RT_E_INVALID otherwise).  rt_device_alloc's pointers are; a sub-buffer at an
 * offset that is no multiple of 8 (16) bytes is not. */
typedef struct rt_noise_state {
    float mean, m2;
} rt_noise_state;

typedef struct rt_noise_summary {
    uint64_t pixels;       /* npix */
    uint64_t above;        /* finite pixels with rel > threshold (rel == threshold is not above) */
    uint64_t nonfinite;    /* non-finite pixels */
    float max_rel_err;     /* the largest rel of the finite pixels (0 when there is none) */
    float reserved;        /* 0 */
} rt_noise_summary;

/* The DEVICE buffer the path modes' renders update: indexed exactly as accum_rgba32f
 * (rt_render: region.w*region.h states, row-major over the region; rt_render_tiles:
 * rt_tileset_local_tiles()*64 packed states, padding slots neither read nor written).
 * It is updated after every fold, on the fold's stream (RT_OPT_ASYNC_FOLD: read it as
 * accum is read).  NULL: off (the default; a render then issues the launches it issues
 * without this call).  Every other mode leaves the buffer untouched, W7E1 and W7E2
 * (which fold inside their kernel and write no records) included. */
int rt_set_noise_buffer(rt_ctx* ctx, rt_noise_state* state_dev);

/* The same kernel over caller-supplied DEVICE records (float4 each: rgb, w ignored) of
 * iterations first_iter .. first_iter+spp-1 for npix pixels: [pixel][iteration] when
 * pixel_major is non-zero, else [iteration][pixel] with stride npix.  npix == 0 or
 * spp == 0: no-op.  Asynchronous on the context stream.  It reads every record it is
 * given: the renders' own scratch holds no records for the pixels RT_OPT_EMPTY_PIXELS
 * flags (their fold and noise update take the constant), so a caller that feeds records
 * of its own supplies them for every pixel. */
int rt_noise_accumulate(rt_ctx* ctx, const float* samples_rgba_dev, uint32_t npix, uint32_t spp,
                        int pixel_major, uint32_t first_iter, rt_noise_state* state_dev);

/* rel_dev[i] (DEVICE, npix floats) = rel of state_dev[i] after n iterations.  RT_E_INVALID
 * for n < 2 or a floor that is not > 0.  Asynchronous on the context stream. */
int rt_noise_map(rt_ctx* ctx, const rt_noise_state* state_dev, uint32_t npix, uint32_t n, float floor,
                 float* rel_dev);

/* The frame's summary into *out (host; synchronizes).  Deterministic: integer counts and
 * an integer maximum of bit patterns, no float atomics.  RT_E_INVALID for n < 2, a floor
 * that is not > 0 or a NaN threshold. */
int rt_noise_summarize(rt_ctx* ctx, const rt_noise_state* state_dev, uint32_t npix, uint32_t n,
                       float threshold, float floor, rt_noise_summary* out);

/* ---- adaptive sampling of the path modes (DESIGN.md section 4 "Adaptive sampling") ----
 * With a per-slot sample-count buffer set, a path-mode render traces and folds only the
 * output slots that are still LIVE; a frozen slot keeps its accumulation, primary id,
 * noise state and count untouched.  No reference counterpart.
 * State per output slot, indexed exactly as accum_rgba32f: the rt_noise_state of the noise
 * buffer (which must be set) and a uint32 count, the iterations folded into the slot.
 * The live set is decided ONCE per rt_render / rt_render_tiles call, at its start, from
 * the state and the counts the previous calls left -- never per pass, so it does not
 * depend on RT_OPT_SAMPLE_BUDGET_MB, the chunk size, the unit order or a probe launch.
 * For a call (first_iter, spp):
 *   first_iter == 0: every valid slot is live; its state and count restart.
 *   first_iter > 0:  a valid slot WANTS MORE iff all of
 *       count == first_iter        it took part in every call so far (a slot that fell
 *                                  behind is frozen for good);
 *       its state is finite        (Welford keeps a NaN: no further sample repairs it; the
 *                                  slot stays reported as non-finite);
 *       first_iter < min_samples, or rel > target, rel being the relative standard error
 *                                  pinned above with n = first_iter and this floor, and the
 *                                  same strict > as rt_noise_summarize's "above".
 *   vote RT_ADAPT_PIXEL: a slot is live iff it wants more.
 *   vote RT_ADAPT_TILE:  a valid slot is live iff its count == first_iter and any slot of
 *       its 8x8 tile wants more.  The tile is the launch's pixel slots 64 t .. 64 t + 63 (one
 *       wave of the kernels: in region mode the 8x8 tiles of the region from its corner, in
 *       tileset mode the packed tile).  A frozen tile stays frozen.  This guards against
 *       the bias of stopping per pixel: a pixel whose first min_samples samples happened to
 *       agree (a dark pixel that a rare bright path reaches) shows no variance yet and
 *       would be frozen too dark; its neighbours, which see the same light, keep it alive.
 *   After the call every live slot has count = first_iter + spp.
 * Invariant: after any sequence of adaptive calls each valid slot p holds, bit for bit, the
 * accumulation, primary id and noise state a uniform render of count[p] iterations gives it
 * (the sample seed is tea16(pixel, iteration) and the average is sequential per pixel).
 * Work: the BSP walk's k_path deals work units for the live slots only (the ascending list
 * of live slots that are not flagged by RT_OPT_EMPTY_PIXELS); with no such slot it is not
 * launched.  Two cases take no list -- the BVH walk, and W7E3 on the BSP walk under
 * RT_BSP_CULL_FAST or RT_BSP_CULL_OFF (its fast-margin kernel sits on its register budget):
 * there k_path traces every slot as without the buffer and the fold skips the slots that
 * are not live.  The frame is the same; no time is saved (rt_adaptive_in_use tells).
 * With the buffer set, rt_last_counts reports the rays actually traced (nothing is added
 * for the pixels RT_OPT_EMPTY_PIXELS flags) and rt_last_elided_primaries counts the flagged
 * pixels that are live only. */
#define RT_ADAPT_PIXEL 0
#define RT_ADAPT_TILE 1

typedef struct rt_adaptive_summary {
    uint64_t pixels;         /* width * height */
    uint64_t live_next;      /* the slots that would be live in a call with first_iter = iteration */
    uint64_t above;          /* finite slots with count >= 2 and rel (n = count) > target */
    uint64_t nonfinite;      /* slots with a non-finite state or count < 2 */
    uint64_t total_samples;  /* the sum of the counts */
    float max_rel_err;       /* the largest rel of the finite slots (0 when there is none) */
    uint32_t min_count, max_count;
    uint32_t reserved;       /* 0 */
} rt_adaptive_summary;

/* count_dev: DEVICE, indexed as accum_rgba32f (rt_render_tiles' packed layout included:
 * padding slots are neither read nor written), 4-byte aligned; NULL: off (the default; a
 * render then issues exactly the launches it issues without this call).  RT_E_INVALID for
 * min_samples < 2, a target that is negative or NaN, a floor that is not > 0, a vote that is
 * neither RT_ADAPT_PIXEL nor RT_ADAPT_TILE, or a misaligned pointer (the parameters are
 * not checked when count_dev is NULL).  A path-mode render with the buffer set and no noise
 * buffer returns RT_E_NOT_READY, and together with RT_OPT_ASYNC_FOLD RT_E_UNSUPPORTED (the
 * live set is read back on the context stream).  Such a render synchronizes the context
 * stream once, at its start.  Every other mode ignores the buffer. */
int rt_set_adaptive(rt_ctx* ctx, uint32_t* count_dev, float target, float floor, uint32_t min_samples, int vote);

/* The fused fold over caller-supplied DEVICE records (rt_noise_accumulate's layouts and
 * alignment; accum_dev 16-byte, state_dev 8-byte, count_dev 4-byte aligned): for every
 * pixel i < npix with live_dev[i] != 0 (one byte per pixel), the progressive average of
 * rt_render into accum_dev[i], the primary id (the record's w bits) of the last iteration
 * into ids_dev[i] (or NULL), the noise update into state_dev[i] and, when last_pass is
 * non-zero, count_dev[i] = first_iter + spp.  first_iter == 0 starts from zero, else the
 * stored accumulation and state continue.  Every other pixel keeps what the four buffers
 * held.  npix == 0 or spp == 0: no-op.  Asynchronous on the context stream. */
int rt_adaptive_accumulate(rt_ctx* ctx, const float* samples_rgba_dev, uint32_t npix, uint32_t spp, int pixel_major,
                           uint32_t first_iter, int last_pass, const uint8_t* live_dev, float* accum_dev,
                           uint32_t* ids_dev, rt_noise_state* state_dev, uint32_t* count_dev);

/* rel_dev[i] (DEVICE, npix floats) = rel of state_dev[i] with n = count_dev[i]; the quiet NaN
 * 0x7FC00000 for a non-finite state or a count < 2.  Asynchronous on the context stream. */
int rt_adaptive_map(rt_ctx* ctx, const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t npix,
                    float floor, float* rel_dev);

/* The summary of a row-major width x height frame (a full-region rt_render's buffers) into
 * *out (host; synchronizes): every rel with n = the slot's own count; live_next by the rule
 * above for a call that starts at `iteration`, with the 8x8 tiles of the frame.
 * Deterministic: integer sums and integer maxima of bit patterns.  Arguments as
 * rt_set_adaptive's. */
int rt_adaptive_summarize(rt_ctx* ctx, const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t width,
                          uint32_t height, uint32_t iteration, float target, float floor, uint32_t min_samples,
                          int vote, rt_adaptive_summary* out);

/* The most recent path-mode render with the count buffer set: *live_slots (or NULL) the
 * slots that were live, *dealt_slots (or NULL) the slots k_path dealt work units for (the
 * live ones that RT_OPT_EMPTY_PIXELS does not flag when it took the list; every slot of the
 * launch in the two fallback cases; 0 when it was not launched), *took_list (or NULL) 1
 * when k_path ran from the list (or was not launched because the list was empty), 0 in a
 * fallback case.  All 0 when the most recent render did not use the buffer. */
int rt_adaptive_in_use(rt_ctx* ctx, uint64_t* live_slots, uint64_t* dealt_slots, int* took_list);

/* ---- denoise: a variance-guided a-trous filter (DESIGN.md section 4 "Denoise") ----
 * An edge-avoiding a-trous wavelet filter (the spatial half of SVGF) over a row-major
 * width x height frame, guided by the variance the noise estimate keeps and by the geometry
 * under each pixel.  No reference counterpart; off unless called.  Pinned f32 arithmetic (no
 * contraction, correctly rounded / and sqrt), every line below one operation, sums left to
 * right; max(a, 0) is (a > 0 ? a : 0), which also sends a NaN to 0; |a| clears the sign bit;
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *
 * Variance (rt_denoise_variance).  With cnt = count[p] (or the call's n without counts) and
 * nf = (float)cnt:
 *     v = (m2 < 0 ? 0 : m2) / (nf * (nf - 1.0f))          the variance of the mean luminance
 * and v = the quiet NaN 0x7FC00000 when cnt < 2 or a field of the state is not finite.
 *
 * Filterable.  At every level a pixel is FILTERABLE iff its three colour components and its v
 * are finite and v is not negative; else it is unfilterable.  As a centre an unfilterable pixel
 * is copied through, colour and v unchanged, at every level; as a tap it has weight 0.
 *
 * Guide (rt_denoise_guide).  The camera is the uniforms' (get_camera_ray, w7e3.wgsl:211-228):
 *     v = normalize(look_at - pos); b1 = normalize(cross(v, up)); b2 = cross(b1, v)
 *     ux = ((float)x + 0.5f) / (float)width - 0.5f;  uy = 0.5f - ((float)y + 0.5f) / (float)height
 *     w(x, y) = normalize(((b1 * (ux + 0.0f)) * aspect + b2 * (uy + 0.0f)) + v * camera_constant)
 * the pixel-centre ray (e, w), e = camera_pos; normalize(a) = a / sqrtf(dot(a, a)).  For the
 * triangle id = ids[p] with vertices v0, v1, v2:
 *     e0 = v1 - v0; e1 = v2 - v0; g = normalize(cross(e0, e1)); if (dot(g, w) > 0) g = -g
 *     den = dot(w, g); num = dot(v0 - e, g); z = num / den
 *     dzx = num / dot(w(x+1, y), g) - z;  dzy = num / dot(w(x, y+1), g) - z
 * (the neighbour's ray is computed as written even when it lies outside the frame); a dzx or
 * dzy that is not finite becomes 0.  The pixel is BACKGROUND when id is 0xFFFFFFFF or >= ntris,
 * den == 0, or z is not finite or <= 0: then N = 0, z = -1, dz = 0.  Else N = g.
 * rt_denoise_filter takes any guide: a pixel is background iff !(z > 0).
 *
 * One level i = 0 .. levels-1 (1 <= levels <= 5) has step s = 2^i, reads the previous level's
 * colour c and variance v (level 0: the inputs) and the same guide, and for a filterable p:
 *   1. sk = sv = 0; for dy = -1..1, dx = -1..1 (dy outer), q = p + (dx, dy) inside the frame
 *      and filterable:  k = ((float)(2-|dy|) * (float)(2-|dx|)) / 16.0f;  sk = sk + k;
 *      sv = sv + k * v_q.   sd = sqrtf(sv / sk)              (the centre counts: sk >= 1/4)
 *   2. h = {1/16, 1/4, 3/8, 1/4, 1/16}; the 25 taps q = p + s*(dx, dy), dy outer, dx inner, both
 *      -2..2.  A tap outside the frame, unfilterable, or of the other class (background against
 *      surface) has weight 0 and adds nothing.  The centre tap has w = h[2] * h[2].  Every other:
 *          d  = dot(N_p, N_q);  wn = max(d, 0), squared seven times (^128)
 *          gr = dzx_p * (float)(s*dx) + dzy_p * (float)(s*dy)
 *          xz = |z_p - z_q| / (sigma_z * |gr| + 1e-3f * |z_p|)
 *          (a background pair: wn = 1, xz = 0)
 *          l  = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z     (the noise estimate's luminance)
 *          xl = |l_p - l_q| / (sigma_l * sd + 1e-6f)
 *          t  = max(1.0f - (xz + xl) * 0.125f, 0), squared three times: E(x) = t^8
 *          w  = ((h[dy+2] * h[dx+2]) * wn) * E
 *      E follows exp(-x) (it is (1 - x/8)^8), has compact support (0 from x = 8 on) and needs
 *      no transcendental.  No weight is NaN: both denominators are positive for a filterable
 *      pair (sigma_l * sd >= 0 plus 1e-6f; for a surface pixel z_p > 0, so 1e-3f * |z_p| > 0
 *      unless it underflows -- and then a NaN or infinite x still gives t = 0 by the max).
 *      Per tap, in order:  sw = sw + w;  sc = sc + w * c_q (per component);  sv = sv + (w*w) * v_q
 *   3. c' = sc / sw;  v' = sv / (sw * sw).  The last level's output alpha is 1.
 * Values whose sums overflow keep their class (infinite or NaN), not a NaN's payload.
 * Defaults of the hosts: levels = 5, sigma_l = 4, sigma_z = 1.
 *
 * All four calls are asynchronous on the context stream, take DEVICE pointers, and return
 * RT_E_INVALID for a null buffer (out_var_dev and count_dev may be NULL), levels outside 1..5,
 * a sigma that is not > 0, n < 2 without counts, a pointer that is not aligned (16 B for the
 * float4 buffers, 8 B for states and dz, 4 B otherwise), an output that overlaps an input or
 * another output, or width * height >= 2^31.  A zero-sized frame is a no-op (RT_OK). */

/* nz_dev: width*height float4 {N.xyz, z}; dz_dev: width*height float2 {dzx, dzy}; from ids_dev
 * (width*height u32, rt_render's primary_hit_ids), the uploaded mesh and the current uniforms,
 * whose resolution must be width x height (RT_E_INVALID otherwise).  RT_E_NOT_READY without a
 * mesh or uniforms. */
int rt_denoise_guide(rt_ctx* ctx, uint32_t width, uint32_t height, const uint32_t* ids_dev, float* nz_dev,
                     float* dz_dev);

/* var_dev[i] (npix floats) = v of state_dev[i] with count_dev[i] (or, count_dev NULL, n) iterations. */
int rt_denoise_variance(rt_ctx* ctx, const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t npix,
                        uint32_t n, float* var_dev);

/* `levels` levels over color_dev (float4: rgb, w ignored) and var_dev into out_color_dev (float4,
 * alpha 1) and out_var_dev (or NULL).  The levels ping-pong between two buffers of the context
 * (allocated at the first call, freed with the context). */
int rt_denoise_filter(rt_ctx* ctx, uint32_t width, uint32_t height, const float* color_dev, const float* var_dev,
                      const float* nz_dev, const float* dz_dev, uint32_t levels, float sigma_l, float sigma_z,
                      float* out_color_dev, float* out_var_dev);

/* The three calls above on the context's scratch: the frame rt_render left in accum_dev, ids_dev
 * and state_dev (the noise buffer) after n iterations -- or count_dev[i] iterations per pixel
 * under adaptive sampling -- filtered into out_rgba_dev.  The inputs are not written.  The
 * primary id is the LAST iteration's: the camera ray's jitter stays inside the pixel, so the
 * id picks one of the surfaces the pixel sees. */
int rt_denoise(rt_ctx* ctx, uint32_t width, uint32_t height, const float* accum_dev, const uint32_t* ids_dev,
               const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t n, uint32_t levels,
               float sigma_l, float sigma_z, float* out_rgba_dev);

/* With RT_OPT_KERNEL_TIMING: the device time of each level of the most recent rt_denoise_filter
 * or rt_denoise in milliseconds (level_ms: 5 floats, 0 past its levels) and the form the level
 * ran (lds_form: 5 uint32, or NULL: 0 every tap from global memory, 1 the LDS tile, 2 the lattice).  Synchronizes.  All 0 when the option was off. */
int rt_denoise_level_times(rt_ctx* ctx, float* level_ms, uint32_t* lds_form);

/* ---- temporal accumulation: reprojected history across camera moves (DESIGN.md section 4
 * "Temporal accumulation") ----
 * The temporal half of SVGF for the path modes: the previous frame's integrated colour, the
 * moments of its luminance and its history length are carried to the new camera by
 * reprojecting the primary hit, rejected where the new pixel does not see them, and blended
 * with the new frame; rt_temporal_variance turns the moments into the variance
 * rt_denoise_filter takes.  No reference counterpart; off unless called.  Pinned f32
 * arithmetic as "denoise" (no contraction, correctly rounded / and sqrt, every line one
 * operation, sums left to right, max(a, 0) = (a > 0 ? a : 0), |a| clears the sign bit,
 * dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; a vector line is that operation per component).
 *
 * Frames.  The sample seed is tea16(pixel, iteration), so frame t of a sequence renders the
 * iterations [k, k + spp), k = t * spp, into a ZEROED accumulation: the progressive fold then
 * leaves A = (sum of the samples) / (k + spp), and the frame's mean is
 *     cur = A.rgb * color_scale,   color_scale = (float)(k + spp) / (float)spp   (the host's)
 * (no noise buffer on such a render: its Welford state would be wrong for first_iter > 0).
 *     l = (0.2126f*cur.x + 0.7152f*cur.y) + 0.0722f*cur.z;   l2 = l * l
 *
 * History of one frame: hist_color float4 {rgb, 1}, hist_mom float2 {m1, m2} (the integrated
 * luminance and its square), hist_len u32, hist_nz float4 (that frame's {N, z} of
 * rt_denoise_guide), all row-major width x height, and the rt_uniform it was rendered with.
 * A camera (e, v, b1, b2, cc, aspect) and its pixel-centre ray w(x, y) are the uniform's, exactly
 * as "denoise / Guide" pins them; primed names are the previous uniform's.
 *
 * rt_temporal_accumulate, pixel p = (x, y) with guide {N_p, z_p}:
 *   1. NO HISTORY when the history pointers are NULL, !(z_p > 0) (background), or a component
 *      of cur is not finite.
 *   2. P = e + w(x, y) * z_p;   d = P - e'
 *   3. a = dot(d, v');  no history unless a > 0
 *   4. ux = ((dot(d, b1') * cc') / a) / aspect';   uy = (dot(d, b2') * cc') / a
 *      fx = (ux + 0.5f) * (float)width - 0.5f;     fy = (0.5f - uy) * (float)height - 0.5f
 *      no history unless fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height
 *      (false for a NaN)
 *   5. x0 = floorf(fx); tx = fx - x0;  y0 = floorf(fy); ty = fy - y0
 *   6. the four taps q = (x0 + i, y0 + j), j outer, i inner, both 0..1:
 *          bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty)
 *      A tap is VALID iff it lies inside the frame, bw > 0, len'_q >= 1, z'_q > 0, the three
 *      components of c'_q and both of m'_q are finite, dot(N_p, N'_q) >= normal_min, and
 *          P_q = e' + w'(q) * z'_q;   |dot(P_q - P, N_p)| <= plane_tol * z_p
 *      (the distance of the tap's own surface point from p's tangent plane: it stays correct at
 *      grazing angles, where a depth ratio does not).
 *   7. sw = sc = sm = 0, nh = 0xFFFFFFFF; per valid tap, in order:
 *          sw = sw + bw;  sc = sc + bw * c'_q;  sm = sm + bw * m'_q;  nh = min(nh, len'_q)
 *      no history unless sw > 0
 *   8. with history:  h = sc / sw;  hm = sm / sw
 *          n = nh >= max_history ? max_history : nh + 1;   al = 1.0f / (float)n
 *          c = h + (cur - h) * al;  m1 = hm.x + (l - hm.x) * al;  m2 = hm.y + (l2 - hm.y) * al
 *          len = n
 *   9. without:  c = cur, {m1, m2} = {l, l2}, len = 1.  A cur that is not finite therefore stays
 *      one pixel: it is copied, its moments are not finite (rt_temporal_variance then gives the
 *      quiet NaN and the filter treats it as unfilterable), and as a tap it is not valid.
 *  10. out_color = {c, 1}, out_mom = {m1, m2}, out_len = len.  The caller keeps the current nz
 *      beside them as the next frame's hist_nz.
 * STILL CAMERA.  When the previous uniform's eleven camera floats (camera_pos, camera_constant,
 * camera_look_at, aspect_ratio, camera_up) are bit-equal to the current ones, steps 3 to 5 are
 * skipped and the only tap is q = p with bw = 1.0f, under the same validity tests: a camera that
 * stands still gives exactly the running mean above, up to max_history frames.  The host
 * decides this per call.  The uniforms' resolutions must both be width x height.
 * Defaults of the hosts: max_history = 32, normal_min = 0.9, plane_tol = 0.01.
 *
 * rt_temporal_variance: the variance of the integrated mean luminance, for rt_denoise_filter.
 * With {m1, m2} = mom[p], len = len[p], the guide {N_p, z_p}, {dzx_p, dzy_p}:
 *     v = the quiet NaN 0x7FC00000 when m1 or m2 is not finite; else
 *     (M1, M2) = (m1, m2) when len >= min_len; else the plain mean over the 7 x 7 neighbourhood:
 *         s1 = s2 = 0, cnt = 0; for dy = -3..3, dx = -3..3 (dy outer), q = p + (dx, dy); the centre
 *         counts; any other q counts iff it lies inside the frame, both its moments are finite, it
 *         is of p's class (background iff !(z > 0)), and for a surface pair
 *             dot(N_p, N_q) >= normal_min  and
 *             |z_p - z_q| <= 2.0f * |dzx_p * (float)dx + dzy_p * (float)dy| + plane_tol * |z_p|
 *         s1 = s1 + m1_q;  s2 = s2 + m2_q;  cnt = cnt + 1;    M1 = s1 / (float)cnt;  M2 = s2 / (float)cnt
 *     v = max(M2 - M1 * M1, 0) / (float)len
 * A fresh or disoccluded pixel so borrows its neighbours' spread (one sample has none of its
 * own) and is blurred more.  Default min_len = 4.
 *
 * Limits: reprojection follows the primary hit, so what a mirror or glass surface shows lags
 * behind the camera, as in SVGF; background pixels keep no history; the scene is static.  With
 * rt_denoise_guide the analytic W8 balls and the W9E2 / W9E3 holdout plane are background: they
 * keep no history at all, even under a still camera.  With the guide of "denoise / Guide with
 * objects" below they keep one, and what a ball shows lags.
 *
 * Both calls are asynchronous on the context stream, take DEVICE pointers (prev_uniform: host)
 * and follow rt_denoise_filter's argument rules: RT_E_INVALID for a null context or buffer,
 * a pointer that is not aligned (16 B float4, 8 B float2, 4 B otherwise), an output that
 * overlaps an input or another output, width * height >= 2^31, a history of which some
 * pointers (prev_uniform included) are NULL and others not, max_history == 0, min_len == 0, a
 * color_scale, normal_min or plane_tol that is NaN, a plane_tol that is negative,
 * and uniforms (the context's, or prev_uniform) whose resolution is not width x height or whose
 * aspect ratios differ.  RT_E_NOT_READY without uniforms.  A zero-sized frame is a no-op. */
int rt_temporal_accumulate(rt_ctx* ctx, uint32_t width, uint32_t height, const float* color_dev, float color_scale,
                           const float* nz_dev, const rt_uniform* prev_uniform, const float* hist_color_dev,
                           const float* hist_mom_dev, const uint32_t* hist_len_dev, const float* hist_nz_dev,
                           uint32_t max_history, float normal_min, float plane_tol, float* out_color_dev,
                           float* out_mom_dev, uint32_t* out_len_dev);

int rt_temporal_variance(rt_ctx* ctx, uint32_t width, uint32_t height, const float* mom_dev, const uint32_t* len_dev,
                         const float* nz_dev, const float* dz_dev, uint32_t min_len, float normal_min, float plane_tol,
                         float* var_dev);

/* With RT_OPT_KERNEL_TIMING: the device time in milliseconds of the most recent
 * rt_temporal_accumulate and rt_temporal_variance (0 when that call was not timed), and the form
 * the latter ran (or NULL: 0 every neighbour from global memory, 1 the LDS tile).  Synchronizes. */
int rt_temporal_times(rt_ctx* ctx, float* accumulate_ms, float* variance_ms, uint32_t* variance_lds_form);

/* ---- denoise / Guide with objects (DESIGN.md section 4 "Guide with objects") ----
 * rt_render's primary id is set on a mesh hit alone: the two analytic balls of W8E1..W8E3 and
 * the holdout plane y = 0 of W9E2 / W9E3 leave it at 0xFFFFFFFF, and rt_denoise_guide classes
 * their pixels as background.  This guide gives those pixels the object's {N, z} and {dzx, dzy}
 * instead, so that the filter separates them from the environment and temporal accumulation
 * keeps their history.  A new entry point: rt_denoise_guide and rt_denoise are as they were, and
 * the hosts use this guide only when asked (set_guide_objects, --guide-objects).  Pinned f32
 * arithmetic as "denoise": no contraction, correctly rounded / and sqrt, every line one
 * operation, the same dot, normalize, |a| and max; a vector line is that operation per component.
 *
 * The camera and the pixel-centre ray (e, w(x, y)) are exactly those of "denoise / Guide".
 * `objects` is a mask of the RT_GUIDE_* bits below.
 *
 * A pixel whose id is not 0xFFFFFFFF is rt_denoise_guide's, its lines and its bits: a valid id,
 * an id >= ntris (background), and every way such a pixel becomes background there.
 *
 * A pixel whose id is 0xFFFFFFFF tests the objects of the mask on (e, w), w = w(x, y), with the
 * shader's own tests in the shader's order, on the interval [tmin, tmax], tmax = 5000.0f at the
 * start, every accept lowering tmax to its distance; tmin is the path kernels' ETA of the modes
 * that hold the object: 0.01f for the balls, 0.0001f for the plane.
 *   RT_GUIDE_BALLS: the mirror ball C = (420, 90, 370), then the glass ball C = (130, 90, 250),
 *   both of radius r = 90.0f (intersect_sphere, w8e1.wgsl:352-376):
 *       oc = e - C;  a = dot(w, w);  b2 = dot(oc, w);  c = dot(oc, oc) - r * r
 *       D = b2 * b2 - a * c;  no hit when D < 0;  sq = sqrtf(D)
 *       t = (-b2 - sq) / a;  if (t < tmin || t > tmax) t = (-b2 + sq) / a
 *       no hit when that t < tmin || t > tmax;  else accepted: tmax = t
 *   RT_GUIDE_PLANE, after the balls: the plane y = 0, n = (0, 1, 0) (intersect_plane,
 *   w9e2.wgsl:388-404):
 *       pn = ((0.0f - e.x) * 0.0f + (0.0f - e.y) * 1.0f) + (0.0f - e.z) * 0.0f
 *       pd = (w.x * 0.0f + w.y * 1.0f) + w.z * 0.0f
 *       t = pn / pd;  accepted iff !(t < tmin) && !(t > tmax) && t is finite && t > 0 && pd != 0
 *       then tmax = t
 *   (the shader accepts a NaN distance; the guide makes no surface of it: such a test accepts
 *   nothing and an earlier ball stays).
 * With no accept the pixel is BACKGROUND, as in rt_denoise_guide: N = 0, z = -1, dz = 0.  Else,
 * for the last accepted object at distance t = tmax:
 *       a ball:  P = e + w * t;  N = normalize(P - C)           the plane:  N = (0, 1, 0)
 *       if (dot(N, w) > 0) N = -N                     (an eye inside a ball or below the plane)
 *       z = t;  den = dot(w, N);  num = z * den
 *       dzx = num / dot(w(x+1, y), N) - z;  dzy = num / dot(w(x, y+1), N) - z
 * the tangent plane at P under the neighbours' rays, as the triangles' lines; a dzx or dzy that
 * is not finite becomes 0.
 *
 * rt_guide_objects names the mask of a mode: RT_GUIDE_BALLS for W8E1..W8E3, RT_GUIDE_PLANE for
 * W9E2 and W9E3, 0 for every other rt_mode (W6E3 has the balls but no primary-id guide: it is no
 * path mode); RT_E_INVALID for a value that is no rt_mode or a null pointer.
 *
 * Limits: the centre ray decides the object, the last iteration's jittered ray the id: at an
 * object's silhouette the two may disagree by a pixel.  What a mirror or glass ball shows lags
 * behind the camera, as any reflection does under "temporal accumulation". */
#define RT_GUIDE_BALLS 1u /* the mirror and the glass ball of W8E1..W8E3 */
#define RT_GUIDE_PLANE 2u /* the holdout plane y = 0 of W9E2 and W9E3 */

int rt_guide_objects(int mode, uint32_t* objects);

/* rt_denoise_guide with the objects of the mask under the pixels that have no id.  Arguments,
 * alignment, overlap and readiness rules are rt_denoise_guide's; RT_E_INVALID also for a bit
 * outside RT_GUIDE_BALLS | RT_GUIDE_PLANE.  objects == 0 gives rt_denoise_guide's bytes. */
int rt_denoise_guide_objects(rt_ctx* ctx, uint32_t objects, uint32_t width, uint32_t height, const uint32_t* ids_dev,
                             float* nz_dev, float* dz_dev);

/* rt_denoise with that guide; every other argument and rule is rt_denoise's. */
int rt_denoise_objects(rt_ctx* ctx, uint32_t objects, uint32_t width, uint32_t height, const float* accum_dev,
                       const uint32_t* ids_dev, const rt_noise_state* state_dev, const uint32_t* count_dev, uint32_t n,
                       uint32_t levels, float sigma_l, float sigma_z, float* out_rgba_dev);

/* ---- multi-GPU: the tile gather over RCCL -----------------
 * One process per GPU, each with its own context: every rank renders its
 * interleaved tiles (rt_render_tiles with rt_tileset {rank, nranks}), then
 * rt_gather_tiles collects them on rank 0 -- one grouped RCCL receive of each
 * peer's packed accumulation (16 B/px) and primary-hit ids (4 B/px), point to
 * point over xGMI, no other collective -- and scatters them into rank 0's frame
 * (rt_unpack_tiles).  Replaces, for a Rust host that tiles one
 * RenderState::render (src/render_state.rs:483-561, driven per frame by
 * src/lib.rs:331-363) across the GPUs of a node, what bench.py did with
 * torch.distributed.  RCCL is loaded at rt_comm_init (librccl.so.1; a process
 * that already holds one, e.g. through PyTorch, shares it). */
#define RT_COMM_ID_BYTES 128u

/* A new communicator id (ncclGetUniqueId), made on rank 0 and handed to every
 * rank out of band (a file, a socket, the launcher's store). */
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);

/* Join the communicator `id` as `rank` of `nranks` on the context's device
 * (ncclCommInitRank; collective: every rank calls it).  One communicator per
 * context; rt_comm_destroy (or rt_destroy) releases it. */
int rt_comm_init(rt_ctx* ctx, uint32_t nranks, uint32_t rank, const uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_destroy(rt_ctx* ctx);

/* Gather the ranks' packed tiles of a width x height frame (each rank:
 * rt_tileset_local_tiles(width, height, nranks) * 64 px in local_accum /
 * local_ids, device pointers) to rank 0 and unpack them into rank 0's
 * row-major frame_accum (W*H RGBA32F) and frame_ids (W*H u32); the other ranks
 * pass NULL frames.  Collective over the context's communicator, asynchronous
 * on the context's stream (RCCL runs on it); the frame is complete once the
 * stream has drained.  Either id pointer may be NULL on every rank (accum only). */
int rt_gather_tiles(rt_ctx* ctx, uint32_t width, uint32_t height, const float* local_accum,
                    const uint32_t* local_ids, float* frame_accum, uint32_t* frame_ids);

/* ---- the trace stage of a wavefront renderer ---------------------------------
 * rt_trace_batch walks n device-resident rays through the context's BSP with the
 * render kernels' step function in a traversal-only persistent kernel (no
 * shading state; refills by ballot + mbcnt from per-XCD queues): rays_dev = n x
 * {o.xyz, w.xyz, tmin, tmax} (f32, rt_trace_rays' layout), flags_dev = n x u32 (bit 0: any-hit, the
 * shadow walk; NULL: every ray closest-hit), hits_dev = n x {u32 record byte
 * offset of the accepted triangle (closest hit), 0xFFFFFFFE (any-hit: blocked) or
 * 0xFFFFFFFF (miss), f32 dist}.  The results are rt_trace_rays' walks (same
 * culling mode).  Asynchronous on the context stream; timed by
 * RT_OPT_KERNEL_TIMING like the render kernels.  RT_OPT_SHADE_THRESHOLD's low
 * byte (default 16) is the lanes-still-tracing count at which finished lanes
 * refill.  n must stay below 2^31 (the per-XCD work queues count 64-ray blocks in
 * 32-bit heads; RT_E_INVALID above).  DESIGN.md section 4 "Outside the megakernel".
 *
 * rt_set_ray_capture arms a capture: every counting render (RT_OPT_DETAIL_COUNTERS)
 * of a W7E3 / W9E1 path mode appends each ray its walks start -- camera, shadow
 * and bounce rays, in issue order -- to rays_dev / flags_dev in the layout above
 * (up to cap rays; NULL disarms); rt_ray_capture_count returns how many were
 * traced since it was armed (more than cap: the rest were not written). */
int rt_trace_batch(rt_ctx* ctx, rt_traverse trav, const float* rays_dev, const uint32_t* flags_dev, uint32_t n,
                   uint32_t* hits_dev);
int rt_set_ray_capture(rt_ctx* ctx, float* rays_dev, uint32_t* flags_dev, uint64_t cap);
int rt_ray_capture_count(rt_ctx* ctx, uint64_t* n);

/* ---- ray queries: the walk alone ------------------------------------------ */

/* One walk per ray through the context's BSP or BVH, with the render kernels'
 * own traversal step: intersect_trimesh (res/shaders/bsp.wgsl:10-81) /
 * intersect_bvh (bvh.wgsl:154-191) for a closest-hit ray; with bit 0 of
 * flags[i] set, the any-hit walk of the shadow and occlusion rays (it stops at
 * the first accepted triangle, as intersect_trimesh_immediate_return,
 * bsp.wgsl:83-155, does).  The query form of the reference's CPU walk
 * intersect_bsp_array (js/bsp_tree/modules/BspTree_interleaved.js:287-352).
 *   rays:  DEVICE, n x 8 floats: origin.xyz, direction.xyz, tmin, tmax;
 *   flags: DEVICE, n u32, or NULL (all closest-hit);
 *   hits:  DEVICE, n x rt_ray_hit.
 * Asynchronous on the context stream. */
typedef struct rt_ray_hit {
    uint32_t tri;          /* the accepted triangle (the last accept), UINT32_MAX on a miss */
    float dist;            /* its distance (the ray's tmax when the walk ends) */
    float beta, gamma;     /* its barycentrics (0 for an any-hit walk, which keeps none) */
    uint32_t ntested;      /* triangles tested, in walk order */
    uint32_t tested_fnv;   /* FNV-1a 32 of the tested triangle ids (little-endian u32) in order */
    float tmin, tmax;      /* the ray interval the walk leaves behind (bsp.wgsl narrows it in place) */
} rt_ray_hit;
int rt_trace_rays(rt_ctx* ctx, rt_traverse trav, const float* rays, const uint32_t* flags, uint32_t n,
                  rt_ray_hit* hits);

/* Counters of the most recent launch (synchronizes).  With rt_set_adaptive's buffer set: the
 * rays actually traced. */
int rt_last_counts(rt_ctx* ctx, rt_ray_counts* counts);

/* Shadow rays of the most recent launch that the path kernel resolved at shading
 * time instead of walking (synchronizes): a lambertian hit whose blocked and
 * unblocked radiance sums are the same bit patterns -- every W9E1 hit, whose light
 * is light_init()'s l_i = 0 -- casts a shadow ray that cannot change the pixel.
 * The W9 modes elide such rays.  They stay counted in rt_ray_counts.shadow (the
 * rays the reference's shader casts), so shadow - elided is what walked the
 * mesh (less the rays the W9 plane stopped).  Filled by the counting instantiation
 * only: 0 when RT_OPT_DETAIL_COUNTERS is off. */
int rt_last_elided_shadows(rt_ctx* ctx, uint64_t* elided);

/* Camera rays of the most recent render that RT_OPT_EMPTY_PIXELS did not cast: its
 * flagged pixels x its iterations.  They stay counted in rt_ray_counts.primary and
 * .samples (the rays the reference's shader casts), so primary - elided is what walked
 * the mesh.  Host arithmetic: filled with or without RT_OPT_DETAIL_COUNTERS.  With
 * rt_set_adaptive's buffer set: the flagged pixels that are live x the iterations, and they
 * are not added to rt_ray_counts. */
int rt_last_elided_primaries(rt_ctx* ctx, uint64_t* elided);

/* Device-vs-host self check of the pinned f32 math (sqrt, division, the
 * rt_detmath.h transcendentals) over n inputs in [lo, hi]; returns the number
 * of bit mismatches in *mismatches. */
int rt_selftest_math(rt_ctx* ctx, uint32_t n, float lo, float hi, uint32_t* mismatches);

/* ---- host-side builders (the Rust code above the reference's GPU boundary) */

typedef struct rt_mesh_host rt_mesh_host;   /* owns Mesh arrays (src/mesh.rs:35-41) */
typedef struct rt_mesh_view {
    const float* vertices;     /* nverts x float4 */
    const float* normals;      /* nverts x float4 */
    const uint32_t* indices;   /* ntris x (v0,v1,v2,material) */
    const rt_material* materials;
    const uint32_t* lights;    /* nlights entries, [0] = UINT32_MAX sentinel */
    uint32_t nverts, ntris, nmats, nlights;
} rt_mesh_view;

/* Mesh::from_obj with tobj 4.0 semantics (single_index, fan triangulation,
 * per-group models, MTL Kd/Ka/Ks/illum), src/mesh.rs:78-202. */
int rt_mesh_load_obj(const char* path, rt_mesh_host** out);
/* Wrap caller arrays into a host mesh (copies). normals/materials may be NULL. */
int rt_mesh_from_arrays(const float* pos_vec4, const float* nrm_vec4, uint32_t nverts,
                        const uint32_t* idx_vec4u, uint32_t ntris,
                        const rt_material* mats, uint32_t nmats, rt_mesh_host** out);
/* Deterministic synthetic meshes for the configs the reference cannot supply:
 *   kind 0: displaced-sphere "bunny" stand-in (~ntris triangles, bunny bbox);
 *   kind 1: 10M-style random triangle soup, centres U[-1,1]^3, half-size 0.01;
 *   kind 2: nx x nz grid of copies of `src` translated by `spacing` (instancing
 *           flattened into one mesh; the reference has no instancing). */
int rt_mesh_synth_bunny(uint32_t ntris_target, uint32_t seed, rt_mesh_host** out);
int rt_mesh_synth_soup(uint32_t ntris, uint32_t seed, rt_mesh_host** out);
int rt_mesh_synth_grid(const rt_mesh_host* src, uint32_t nx, uint32_t nz, float spacing,
                       rt_mesh_host** out);
int rt_mesh_scale(rt_mesh_host* m, float factor);   /* Mesh::scale, src/mesh.rs:246-252 */
int rt_mesh_view_get(const rt_mesh_host* m, rt_mesh_view* view);
void rt_mesh_free(rt_mesh_host* m);

typedef struct rt_bsp_host rt_bsp_host;
typedef struct rt_bsp_view {
    const uint32_t* tree;     /* nnodes x vec4u */
    const float* planes;      /* nnodes */
    const uint32_t* ids;      /* nids */
    float aabb[8];            /* BboxGpu */
    uint32_t nnodes, nids, max_depth;
} rt_bsp_view;

/* BspTree::new(bboxes, max_depth, max_leaf) + bsp_array() + primitive_ids(),
 * bit-identical to the reference's f32 arithmetic; nthreads <= 0 = hardware. */
int rt_bsp_build(const rt_mesh_host* mesh, uint32_t max_depth, uint32_t max_leaf,
                 int nthreads, rt_bsp_host** out);
int rt_bsp_view_get(const rt_bsp_host* b, rt_bsp_view* view);
void rt_bsp_free(rt_bsp_host* b);

typedef struct rt_bvh_host rt_bvh_host;
typedef struct rt_bvh_view {
    const rt_gpu_node* nodes;
    const uint32_t* tri_ids;
    uint32_t nnodes, nids;
} rt_bvh_view;

/* hlbvh::Bvh::new(mesh, max_prims) + flatten() + triangles(). Equal Morton
 * codes are ordered by primitive index (the reference's rdst order is
 * implementation-defined). */
int rt_bvh_build(const rt_mesh_host* mesh, uint32_t max_prims, rt_bvh_host** out);
int rt_bvh_view_get(const rt_bvh_host* b, rt_bvh_view* view);
void rt_bvh_free(rt_bvh_host* b);

/* Convenience: upload a host mesh / BSP / BVH built above. */
int rt_upload_mesh_host(rt_ctx* ctx, const rt_mesh_host* m);
int rt_upload_bsp_host(rt_ctx* ctx, const rt_bsp_host* b);
int rt_upload_bvh_host(rt_ctx* ctx, const rt_bvh_host* b);

#ifdef __cplusplus
}
#endif
#endif /* RT02562_RT_H */
