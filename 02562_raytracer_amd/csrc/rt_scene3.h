// rt_scene3.h -- the three-object scene of worksheets 1 to 3 (res/shaders/w1e4.wgsl ..
// w3e4.wgsl): a triangle, a sphere of radius 0.3 and the plane y = 0 as constants, a
// point light at (0, 1.2, 0), the objects' base colours and the background.  The one
// device copy: rt_worksheet1.hip (W1E4..W1E6) and rt_analytic.hip (W2E1..W3E4) render
// the scene, rt_shade.h uses the sphere test for the W8 balls.
//
// Each test answers whether the object is hit inside [tmin, tmax] and at which
// distance; what an accept means is the caller's: the worksheet-1 shaders lower tmax
// to it (the closest hit wins), the W2 / W3 shaders stop at the first accept and pass
// the constant 5000.  Callers compute the position o + w * dist and the normal
// themselves.  The operations and their order are the shaders'.
#pragma once
#include "rt_device_common.h"

namespace rtk {

constexpr float SCENE3_ETA = 0.00001f;    // ray_init's tmin
constexpr float SCENE3_TMAX = 5000.0f;    // and tmax
constexpr float SCENE3_RADIUS = 0.3f;
__device__ __forceinline__ f3 scene3_center() { return V(0.0f, 0.5f, 0.0f); }
__device__ __forceinline__ f3 scene3_plane_normal() { return V(0.0f, 1.0f, 0.0f); }
__device__ __forceinline__ f3 scene3_plane_position() { return V(0.0f, 0.0f, 0.0f); }
// base colours as intersect_scene sets them (W2E2 onwards give the sphere the triangle's)
__device__ __forceinline__ f3 scene3_triangle_color() { return V(0.4f, 0.3f, 0.2f); }
__device__ __forceinline__ f3 scene3_sphere_color() { return V(0.0f, 0.0f, 0.0f); }
__device__ __forceinline__ f3 scene3_plane_color() { return V(0.1f, 0.7f, 0.0f); }
__device__ __forceinline__ f3 scene3_background() { return V(0.1f, 0.3f, 0.6f); }

// The two balls of W8E1..W8E3 (w8e1.wgsl:244-262: the mirror ball, then the glass ball), tested
// with scene3_sphere below: one definition for the path kernel (rt_shade.h w8_balls) and the
// object guide (rt_denoise.hip)
constexpr float W8_BALL_RADIUS = 90.0f;
__device__ __forceinline__ f3 w8_mirror_center() { return V(420.0f, 90.0f, 370.0f); }
__device__ __forceinline__ f3 w8_glass_center() { return V(130.0f, 90.0f, 250.0f); }

struct Scene3Tri {
    f3 v0, e0, e1, normal;   // normal = cross(e0, e1), not normalised
};
__device__ __forceinline__ Scene3Tri scene3_tri()
{
    const f3 v0 = V(0.2f, 0.1f, 0.9f), v1 = V(-0.2f, 0.1f, -0.1f), v2 = V(-0.2f, 0.1f, 0.9f);
    Scene3Tri t;
    t.v0 = v0;
    t.e0 = sub(v1, v0);
    t.e1 = sub(v2, v0);
    t.normal = cross(t.e0, t.e1);
    return t;
}

// intersect_triangle (w1e4.wgsl:164-194, w2e1.wgsl:206-236) on the scene's one triangle
__device__ __forceinline__ bool scene3_triangle(const f3 o, const f3 w, float tmin, float tmax, float& dist)
{
    const Scene3Tri t = scene3_tri();
    const f3 ov = sub(t.v0, o);
    const f3 nom = cross(ov, w);
    const float denom = dot(w, t.normal);
    if (rt_absf(denom) < 1e-6f) return false;
    const float beta = dot(nom, t.e1) / denom;
    const float gamma = -dot(nom, t.e0) / denom;
    const float distance = dot(ov, t.normal) / denom;
    if ((beta < 0.0f) | (gamma < 0.0f) | (beta + gamma > 1.0f) | (distance > tmax) | (distance < tmin)) return false;
    dist = distance;
    return true;
}
// intersect_sphere (w1e4.wgsl:196-222, w2e1.wgsl:238-264, w8e1.wgsl:352-376): the near
// root, or else the far one; the direction of a refracted ray is not a unit vector
__device__ __forceinline__ bool scene3_sphere(const f3 o, const f3 w, float tmin, float tmax, const f3 center,
                                              float radius, float& dist)
{
    const f3 oc = sub(o, center);
    const float a = dot(w, w);
    const float b_over_2 = dot(oc, w);
    const float c = dot(oc, oc) - radius * radius;
    const float discriminant = b_over_2 * b_over_2 - a * c;
    if (discriminant < 0.0f) return false;
    const float disc_sqrt = rt_det_sqrtf(discriminant);
    float root = (-b_over_2 - disc_sqrt) / a;
    if ((root < tmin) | (root > tmax)) {
        root = (-b_over_2 + disc_sqrt) / a;
        if ((root < tmin) | (root > tmax)) return false;
    }
    dist = root;
    return true;
}
// intersect_plane (w1e4.wgsl:149-162, w2e1.wgsl:191-204): the division is unguarded;
// 0 / 0 is NaN, both comparisons are false on it and the plane is accepted with a NaN
// distance
__device__ __forceinline__ bool scene3_plane(const f3 o, const f3 w, float tmin, float tmax, float& dist)
{
    const f3 normal = scene3_plane_normal();
    const float distance = dot(sub(scene3_plane_position(), o), normal) / dot(w, normal);
    if ((distance < tmin) | (distance > tmax)) return false;
    dist = distance;
    return true;
}

// sample_point_light (w1e6.wgsl:239-252): the incident radiance and the direction to the
// light, not normalised
struct Scene3Light {
    f3 l_i, w_i;
};
__device__ __forceinline__ Scene3Light scene3_point_light(const f3 pos)
{
    const f3 intensity = muls(V(RT_PI_F, RT_PI_F, RT_PI_F), 5.0f);
    Scene3Light l;
    l.w_i = sub(V(0.0f, 1.2f, 0.0f), pos);
    const float dist = dot(l.w_i, l.w_i);   // the squared length
    l.l_i = divs(intensity, dist * dist);
    return l;
}

}  // namespace rtk
