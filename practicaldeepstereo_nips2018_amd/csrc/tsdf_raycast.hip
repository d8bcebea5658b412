// TSDF raycast (pds_tsdf_raycast_fwd; not in the reference): the volume of tsdf.hip seen from a pinhole camera, as a depth
// map and a normal map (the model prediction of KinectFusion).
//
// The volume: tsdf and weight, float32 [nz, ny, nx], x fastest; voxel v = (k * ny + j) * nx + i.  In grid coordinates voxel
// (i, j, k) is the point (i, j, k).  Per pose the host gives M (3 x 3), o (3) and R (3 x 3), rounded once to float32: a
// point p of the camera frame lies at the grid position M p + o (the Python mirror: M = R^T / voxel_size,
// o = (-R^T t - origin) / voxel_size - 0.5 for the pose [R | t] from the world into the camera frame).
//
// Per pixel (px, py), in fp32:
//   1. y = (py - cy) / fy, x = ((px - cx) - skew y) / fx, dir = (x, y, 1): the ray parameter s IS the camera Z.
//      d = M dir, g(s) = o + s d.
//   2. [s0, s1]: s clipped to 0 <= g_a <= n_a - 1 on the three axes (slabs) and to [near, far].  A miss if that is empty or
//      not finite, or if any n_a < 2.
//   3. samples s_m = fmaf(m, step, s0), m = 0, 1, ... while s_m <= s1.  At a sample c_a = min(floor(g_a), n_a - 2) (and
//      not below 0: a coordinate a rounding outside the box still reads inside the volume), f_a = g_a - c_a.  The sample is
//      observed when the eight corners of cell c have weight >= min_weight; its value is then the trilinear interpolant of
//      tsdf, in x, then y, then z, each lerp fmaf(t, b - a, a).
//   4. the march stops at the first observed sample whose value is < 0: a hit if sample m - 1 exists, is observed and is
//      not < 0, a miss otherwise (the surface met from behind, or out of unobserved space).  Running past s1 is a miss.
//   5. depth = fmaf(step, v_prev / (v_prev - v_cur), s_prev)
//   6. normal: the analytic gradient of the trilinear interpolant in the cell that contains g(depth), rotated by R, scaled
//      by its largest component and normalised as tsdf_extract_scatter does; NaN where that cell has an unobserved corner or
//      the gradient is zero or not finite (the depth stays).  The tsdf is positive towards the camera, so the normal faces
//      it; the few whose gradient points along the ray instead (n . dir > 0: on noisy data the interpolant need not fall
//      monotonically between two samples) are negated, so that n . dir <= 0 always.
//
// tsdf_raycast: one thread per pixel, a workgroup of 256 threads per 16 x 16 pixel tile, each wave an 8 x 8 block of it
// (not a 64 x 1 row): neighbouring rays walk the same voxels, so the sixteen gathered reads of a sample fall into few cache
// lines, and their marches end at about the same sample.  B * ceil(h / 16) * ceil(w / 16) workgroups; the poses travel in
// the argument struct, kTsdfRaycastPoses per launch.  The march is bounded by kTsdfRaycastMaxSamples whatever the inputs.
// No LDS, no atomics, no workgroup waits on another; the outputs are written once, straight from registers.
// Every multiply-add is an explicit fmaf and contraction is off.
#include "tsdf_ray.hpp"

#pragma clang fp contract(off)

namespace pds {

namespace {

constexpr int kRaycastThreads = 256;
static_assert(kTsdfRaycastTile == 16 && kRaycastThreads == kTsdfRaycastTile * kTsdfRaycastTile, "8 x 8 pixels per wave");

// (raycast_ray, raycast_cell, raycast_corners, raycast_observed, lerp and raycast_value: tsdf_ray.hpp, shared with
// tsdf_color.hip)
template <bool NORMALS>
__global__ __launch_bounds__(kRaycastThreads) void tsdf_raycast_kernel(TsdfRaycastArgs a,
                                                                       const float* __restrict__ tsdf,
                                                                       const float* __restrict__ weight,
                                                                       float* __restrict__ depth,
                                                                       float* __restrict__ normals) {
    const int tiles = a.tiles_x * a.tiles_y;
    const int entry = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - entry * tiles;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int px = tx * kTsdfRaycastTile + (wave & 1) * 8 + (lane & 7);
    const int py = ty * kTsdfRaycastTile + (wave >> 1) * 8 + (lane >> 3);
    if (px >= a.w || py >= a.h) return;
    const int pixel = (entry * a.h + py) * a.w + px;   // (batch * h * w < 2^31)
    const float* pose = a.pose[entry];                 // M (9), o (3), R (9): uniform over the workgroup
    const float nan = __builtin_nanf("");

    // 1. the ray
    float x, y, d[3], o[3];
    raycast_ray(a, pose, px, py, x, y, d, o);

    // 2. the slabs
    float s0 = a.z_near, s1 = a.z_far;
    bool inside = a.nx >= 2 && a.ny >= 2 && a.nz >= 2;
    const float top[3] = {(float)(a.nx - 1), (float)(a.ny - 1), (float)(a.nz - 1)};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (d[m] == 0.f) {
            inside = inside && o[m] >= 0.f && o[m] <= top[m];
        } else {
            const float t0 = (0.f - o[m]) / d[m], t1 = (top[m] - o[m]) / d[m];
            s0 = fmaxf(s0, fminf(t0, t1));
            s1 = fminf(s1, fmaxf(t0, t1));
        }
    }
    const float inf = __builtin_inff();
    inside = inside && s0 <= s1 && s0 > -inf && s1 < inf;   // (a NaN fails)

    // 3., 4. the march
    const int sy = a.nx, sz = a.nx * a.ny;
    float s_prev = 0.f, v_prev = 0.f, hit = nan;
    bool prev_ok = false;
    if (inside) {
        for (int m = 0; m < kTsdfRaycastMaxSamples; ++m) {
            const float s = fmaf((float)m, a.step, s0);
            if (!(s <= s1)) break;
            const float g[3] = {fmaf(s, d[0], o[0]), fmaf(s, d[1], o[1]), fmaf(s, d[2], o[2])};
            float f[3], w[8];
            const int base = raycast_cell(a, g, f);
            raycast_corners(weight, base, sy, sz, w);
            bool ok = false;
            float value = 0.f;
            if (raycast_observed(w, a.min_weight)) {
                float v[8];
                raycast_corners(tsdf, base, sy, sz, v);
                value = raycast_value(v, f);
                if (value < 0.f) {
                    // 5. one linear step between the two samples (v_prev >= 0 > value: the difference is positive)
                    if (prev_ok) hit = fmaf(a.step, v_prev / (v_prev - value), s_prev);
                    break;
                }
                ok = true;
            }
            prev_ok = ok;
            s_prev = s;
            v_prev = value;
        }
    }
    depth[pixel] = hit;
    if (!NORMALS) return;

    // 6. the gradient of the interpolant at g(depth)
    float n[3] = {nan, nan, nan};
    if (hit == hit) {
        const float g[3] = {fmaf(hit, d[0], o[0]), fmaf(hit, d[1], o[1]), fmaf(hit, d[2], o[2])};
        float f[3], w[8];
        const int base = raycast_cell(a, g, f);
        raycast_corners(weight, base, sy, sz, w);
        if (raycast_observed(w, a.min_weight)) {
            float v[8];
            raycast_corners(tsdf, base, sy, sz, v);
            // d/dx: the x differences interpolated in y, then z; d/dy: the y differences of the x lerps, in z; d/dz
            const float gx = lerp(f[2], lerp(f[1], v[1] - v[0], v[3] - v[2]), lerp(f[1], v[5] - v[4], v[7] - v[6]));
            const float c00 = lerp(f[0], v[0], v[1]), c10 = lerp(f[0], v[2], v[3]);
            const float c01 = lerp(f[0], v[4], v[5]), c11 = lerp(f[0], v[6], v[7]);
            const float gy = lerp(f[2], c10 - c00, c11 - c01);
            const float gz = lerp(f[1], c01, c11) - lerp(f[1], c00, c10);
            float r[3], largest = 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                r[m] = fmaf(pose[12 + 3 * m], gx, fmaf(pose[12 + 3 * m + 1], gy, pose[12 + 3 * m + 2] * gz));
                largest = fmaxf(largest, fabsf(r[m]));
            }
            // towards the camera: between two samples the interpolant need not fall monotonically, and where its
            // gradient at g(depth) points along the ray the normal is turned round
            if (fmaf(r[0], x, fmaf(r[1], y, r[2])) > 0.f) {
                r[0] = -r[0];
                r[1] = -r[1];
                r[2] = -r[2];
            }
            // scaled by its largest component first: the squares of a tiny gradient do not vanish
            const bool ok = largest > 0.f && largest < inf && r[0] == r[0] && r[1] == r[1] && r[2] == r[2];
            const float q0 = r[0] / largest, q1 = r[1] / largest, q2 = r[2] / largest;
            const float length = sqrtf(fmaf(q0, q0, fmaf(q1, q1, q2 * q2)));
            if (ok) {
                n[0] = q0 / length;
                n[1] = q1 / length;
                n[2] = q2 / length;
            }
        }
    }
    float* out = normals + 3 * (size_t)pixel;
    out[0] = n[0];
    out[1] = n[1];
    out[2] = n[2];
}

}  // namespace

int tsdf_raycast_groups(int batch, int h, int w) {
    const long long tiles = (long long)((h + kTsdfRaycastTile - 1) / kTsdfRaycastTile) *
                            ((w + kTsdfRaycastTile - 1) / kTsdfRaycastTile);
    return (int)(batch * tiles);
}

int launch_tsdf_raycast(const TsdfRaycastArgs& args, const float* rays, const float* rotations, const float* tsdf,
                        const float* weight, float* depth, float* normals, int batch, hipStream_t s) {
    for (int first = 0; first < batch; first += kTsdfRaycastPoses) {
        const int entries = batch - first < kTsdfRaycastPoses ? batch - first : kTsdfRaycastPoses;
        TsdfRaycastArgs a = args;
        for (int e = 0; e < entries; ++e) {
            for (int k = 0; k < 12; ++k) a.pose[e][k] = rays[12 * (size_t)(first + e) + k];
            for (int k = 0; k < 9; ++k) a.pose[e][12 + k] = rotations[9 * (size_t)(first + e) + k];
        }
        const size_t offset = (size_t)first * a.h * a.w;
        const int groups = tsdf_raycast_groups(entries, a.h, a.w);
        const int probe = probe_before("tsdf_raycast", s);
        if (normals)
            hipLaunchKernelGGL(tsdf_raycast_kernel<true>, dim3(groups), dim3(kRaycastThreads), 0, s, a, tsdf, weight,
                               depth + offset, normals + 3 * offset);
        else
            hipLaunchKernelGGL(tsdf_raycast_kernel<false>, dim3(groups), dim3(kRaycastThreads), 0, s, a, tsdf, weight,
                               depth + offset, static_cast<float*>(nullptr));
        probe_after(probe, groups, s);
        if (int rc = check_launch("tsdf_raycast")) return rc;
    }
    return 0;
}

}  // namespace pds
