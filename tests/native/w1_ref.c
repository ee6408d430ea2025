/* w1_ref.c -- plain C restatement of the worksheet-1 shaders
 * res/shaders/w1e2.wgsl .. w1e5.wgsl, the CPU reference of the RT_MODE_W1E2..W1E5
 * GPU tests.  It shares no code with the kernel
 * (02562_raytracer_amd/csrc/rt_worksheet1.hip): it keeps the shaders' own shape --
 * a Ray and a HitRecord passed by pointer, intersect_scene calling the three tests
 * in turn on the same ray, fs_main's bounce loop -- so that "the closest hit wins",
 * the NaN plane and the single pass of the loop fall out of the data flow instead of
 * being restated as rules.  W1E2 has no ray: its frame is the rasteriser's coverage
 * of the quad scaled by 0.9, restated here in the pinned form (DESIGN.md
 * "Worksheet-1 scenes").
 * Build: gcc -O2 -ffp-contract=off -shared -fPIC (every operation is a single
 * correctly rounded f32 + - * / sqrt, so the result is bit-exact).
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rt.h"

#define ETA 0.00001f
#define NONE 0xFFFFFFFFu
#define MAX_DEPTH 10

typedef struct {
    float direction[3], origin[3];
    float tmax, tmin;
} ray_t;

typedef struct {
    int has_hit;
    int depth;
    float dist;
    float position[3], normal[3];
    float base_color[3];
    uint32_t object;   /* not in the shader: which test wrote base_color last (0, 1, 2) */
} hit_t;

static float v_dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void v_sub(const float* a, const float* b, float* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
static void v_cross(const float* a, const float* b, float* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
static void v_norm(const float* a, float* o)
{
    const float l = sqrtf(v_dot(a, a));
    o[0] = a[0] / l;
    o[1] = a[1] / l;
    o[2] = a[2] / l;
}
static void v_set(float* o, float x, float y, float z) { o[0] = x; o[1] = y; o[2] = z; }

static ray_t ray_init(const float* direction, const float* origin)
{
    ray_t r;
    memcpy(r.direction, direction, sizeof r.direction);
    memcpy(r.origin, origin, sizeof r.origin);
    r.tmax = 5000.0f;
    r.tmin = ETA;   /* w1e3.wgsl has 0.0001 here and never reads it */
    return r;
}
static void ray_at(const ray_t* r, float dist, float* o)
{
    for (int k = 0; k < 3; k++) o[k] = r->origin[k] + r->direction[k] * dist;
}

/* get_camera_ray: w1e3.wgsl and w1e4.wgsl take d = 1.0 and no aspect; w1e5.wgsl reads both */
static ray_t get_camera_ray(const rt_uniform* u, int mode, float uvx, float uvy)
{
    float v[3], b1[3], b2[3], tmp[3], q[3], dir[3];
    v_sub(u->camera_look_at, u->camera_pos, tmp);
    v_norm(tmp, v);
    v_cross(v, u->camera_up, tmp);
    v_norm(tmp, b1);
    v_cross(b1, v, b2);
    if (mode == RT_MODE_W1E5) {
        const float d = u->camera_constant, aspect = u->aspect_ratio;
        for (int k = 0; k < 3; k++) q[k] = b1[k] * uvx * aspect + b2[k] * uvy + v[k] * d;
    } else {
        const float d = 1.0f;
        for (int k = 0; k < 3; k++) q[k] = b1[k] * uvx + b2[k] * uvy + v[k] * d;
    }
    v_norm(q, dir);
    return ray_init(dir, u->camera_pos);
}

static int intersect_plane(ray_t* r, hit_t* hit, const float* normal, const float* position)
{
    const ray_t ray = *r;
    float d[3];
    v_sub(position, ray.origin, d);
    const float distance = v_dot(d, normal) / v_dot(ray.direction, normal);
    if (distance < ray.tmin || distance > ray.tmax) return 0;
    r->tmax = distance;
    hit->dist = distance;
    ray_at(&ray, distance, hit->position);
    memcpy(hit->normal, normal, sizeof hit->normal);
    return 1;
}

static int intersect_triangle(ray_t* r, hit_t* hit, const float v[3][3])
{
    const ray_t ray = *r;
    float e0[3], e1[3], o_to_v0[3], normal[3], nom[3];
    v_sub(v[1], v[0], e0);
    v_sub(v[2], v[0], e1);
    v_sub(v[0], ray.origin, o_to_v0);
    v_cross(e0, e1, normal);
    v_cross(o_to_v0, ray.direction, nom);
    const float denom = v_dot(ray.direction, normal);
    if (fabsf(denom) < 1e-6f) return 0;
    const float beta = v_dot(nom, e1) / denom;
    const float gamma = -v_dot(nom, e0) / denom;
    const float distance = v_dot(o_to_v0, normal) / denom;
    if (beta < 0.0f || gamma < 0.0f || beta + gamma > 1.0f || distance > ray.tmax || distance < ray.tmin) return 0;
    r->tmax = distance;
    hit->dist = distance;
    ray_at(&ray, distance, hit->position);
    v_norm(normal, hit->normal);
    return 1;
}

static int intersect_sphere(ray_t* r, hit_t* hit, const float* center, float radius)
{
    const ray_t ray = *r;
    float oc[3], d[3];
    v_sub(ray.origin, center, oc);
    const float a = v_dot(ray.direction, ray.direction);
    const float b_over_2 = v_dot(oc, ray.direction);
    const float c = v_dot(oc, oc) - radius * radius;
    const float discriminant = b_over_2 * b_over_2 - a * c;
    if (discriminant < 0.0f) return 0;
    const float disc_sqrt = sqrtf(discriminant);
    float root = (-b_over_2 - disc_sqrt) / a;
    if (root < ray.tmin || root > ray.tmax) {
        root = (-b_over_2 + disc_sqrt) / a;
        if (root < ray.tmin || root > ray.tmax) return 0;
    }
    r->tmax = root;
    hit->dist = root;
    ray_at(&ray, root, hit->position);
    v_sub(hit->position, center, d);
    v_norm(d, hit->normal);
    return 1;
}

static int intersect_scene(ray_t* r, hit_t* hit)
{
    static const float arr[3][3] = {{0.2f, 0.1f, 0.9f}, {-0.2f, 0.1f, -0.1f}, {-0.2f, 0.1f, 0.9f}};
    static const float center[3] = {0.0f, 0.5f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f}, origin[3] = {0.0f, 0.0f, 0.0f};
    int has_hit = 0;
    if (intersect_triangle(r, hit, arr)) {
        has_hit = 1;
        v_set(hit->base_color, 0.4f, 0.3f, 0.2f);
        hit->object = 0u;
    }
    if (intersect_sphere(r, hit, center, 0.3f)) {
        has_hit = 1;
        v_set(hit->base_color, 0.0f, 0.0f, 0.0f);
        hit->object = 1u;
    }
    if (intersect_plane(r, hit, up, origin)) {
        has_hit = 1;
        v_set(hit->base_color, 0.1f, 0.7f, 0.0f);
        hit->object = 2u;
    }
    return has_hit;
}

static void shade(ray_t* r, hit_t* hit, float* color)
{
    (void)r;
    hit->has_hit = 1;
    hit->depth += 1;
    memcpy(color, hit->base_color, 3 * sizeof(float));
}

/* The quad scaled by 0.9 covers clip space [-0.9, 0.9]^2, i.e. [0.05 W, 0.95 W) x
 * [0.05 H, 0.95 H) in pixels; pixel x is covered when its centre x + 0.5 lies in that
 * half-open interval (top-left fill rule): 0.05 W <= x + 0.5 < 0.95 W, times 20. */
static int covered(uint32_t x, uint32_t y, uint32_t W, uint32_t H)
{
    const uint64_t cx = 20ull * x + 10ull, cy = 20ull * y + 10ull;
    return cx >= W && cx < 19ull * W && cy >= H && cy < 19ull * H;
}

/* counts: samples, primary, shadow, bounce */
int w1_ref_render(const rt_uniform* u, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int mode, float* accum,
                  uint32_t* ids, uint64_t counts[4])
{
    if (mode < RT_MODE_W1E2 || mode > RT_MODE_W1E5) return -1;
    uint64_t n_samples = 0, n_primary = 0;
    for (uint32_t ry = 0; ry < h; ry++)
        for (uint32_t rx = 0; rx < w; rx++) {
            const uint32_t px = x0 + rx, py = y0 + ry;
            float result[3] = {0.0f, 0.0f, 0.0f};
            uint32_t prim = NONE;
            n_samples++;
            if (mode == RT_MODE_W1E2) {
                /* pixels the quad does not cover keep the clear colour (render_state.rs:506-511) */
                if (covered(px, py, u->resolution[0], u->resolution[1])) v_set(result, 0.1f, 0.3f, 0.6f);
            } else {
                /* uv = coords * 0.5 */
                const float uvx = ((float)px + 0.5f) / (float)u->resolution[0] - 0.5f;
                const float uvy = 0.5f - ((float)py + 0.5f) / (float)u->resolution[1];
                ray_t r = get_camera_ray(u, mode, uvx, uvy);
                n_primary++;
                if (mode == RT_MODE_W1E3) {
                    for (int k = 0; k < 3; k++) result[k] = (r.direction[k] + 1.0f) / 2.0f;
                } else {
                    hit_t hit;
                    memset(&hit, 0, sizeof hit);
                    hit.object = NONE;
                    for (int i = 0; i < MAX_DEPTH; i++) {
                        if (intersect_scene(&r, &hit)) {
                            float c[3];
                            shade(&r, &hit, c);
                            for (int k = 0; k < 3; k++) result[k] += c[k];
                        } else {
                            result[0] += 0.1f;
                            result[1] += 0.3f;
                            result[2] += 0.6f;
                            break;
                        }
                        if (hit.has_hit) break;
                    }
                    prim = hit.object;
                }
            }
            float* o = accum + 4u * ((size_t)ry * w + rx);
            o[0] = result[0];
            o[1] = result[1];
            o[2] = result[2];
            o[3] = 1.0f;
            if (ids) ids[(size_t)ry * w + rx] = prim;
        }
    if (counts) {
        counts[0] = n_samples;
        counts[1] = n_primary;
        counts[2] = 0;
        counts[3] = 0;
    }
    return 0;
}
