/* Brute force for tests/test_pixel_depth.py: every triangle of a mesh through the f32
 * intersect_triangle of w9e1.wgsl:297-339 (as oracle/oracle_render.c tri_test states it:
 * no contraction, the shader's operation order), for many rays, on one interval.  Per
 * ray: how many triangles accept, and the smallest and the largest accepted distance --
 * every accept, not only the closest.  Triangles are structure-of-arrays so that the
 * compiler can vectorise the loop; rays are spread over threads (OpenMP when built with it).
 *
 * gcc -O3 -march=native -ffp-contract=off -fno-fast-math -fopenmp -shared -fPIC */
#include <math.h>
#include <stdint.h>

/* tri: 9 arrays of ntris floats (v0.xyz, v1.xyz, v2.xyz), ray: 6 floats (o, w) each.
 * out: per ray {count, nan_count} and {dmin, dmax} (dmin = +inf, dmax = -inf when none). */
void pdb_accepts(const float* const tri[9], uint32_t ntris, const float* rays, uint32_t nrays, float tmin, float tmax,
                 uint32_t* count, float* dmin_out, float* dmax_out)
{
    const float *restrict t0 = tri[0], *restrict t1 = tri[1], *restrict t2 = tri[2], *restrict t3 = tri[3],
                *restrict t4 = tri[4], *restrict t5 = tri[5], *restrict t6 = tri[6], *restrict t7 = tri[7],
                *restrict t8 = tri[8];
#pragma omp parallel for schedule(dynamic, 64)
    for (uint32_t r = 0; r < nrays; r++) {
        const float ox = rays[6 * r], oy = rays[6 * r + 1], oz = rays[6 * r + 2];
        const float wx = rays[6 * r + 3], wy = rays[6 * r + 4], wz = rays[6 * r + 5];
        float lo = INFINITY, hi = -INFINITY;
        uint32_t n = 0, nn = 0;
#pragma omp simd reduction(min : lo) reduction(max : hi) reduction(+ : n, nn)
        for (uint32_t t = 0; t < ntris; t++) {
            const float ax = t0[t], ay = t1[t], az = t2[t];
            const float e0x = t3[t] - ax, e0y = t4[t] - ay, e0z = t5[t] - az;
            const float e1x = t6[t] - ax, e1y = t7[t] - ay, e1z = t8[t] - az;
            const float px = ax - ox, py = ay - oy, pz = az - oz;   /* o_to_v0 */
            const float nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
            const float mx = py * wz - pz * wy, my = pz * wx - px * wz, mz = px * wy - py * wx;   /* cross(o_to_v0, w) */
            const float denom = wx * nx + wy * ny + wz * nz;
            const float beta = (mx * e1x + my * e1y + mz * e1z) / denom;
            const float gamma = -(mx * e0x + my * e0y + mz * e0z) / denom;
            const float dist = (px * nx + py * ny + pz * nz) / denom;
            const int rej = (fabsf(denom) < 1e-10f) | (beta < 0.0f) | (gamma < 0.0f) | (beta + gamma > 1.0f) |
                            (dist > tmax) | (dist < tmin);
            const int isn = dist != dist;
            n += !rej;
            nn += !rej & isn;
            lo = (!rej & !isn & (dist < lo)) ? dist : lo;
            hi = (!rej & !isn & (dist > hi)) ? dist : hi;
        }
        count[2 * r] = n;
        count[2 * r + 1] = nn;
        dmin_out[r] = lo;
        dmax_out[r] = hi;
    }
}
