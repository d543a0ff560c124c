// Closest point on a triangle, shared by the mesh operator (nn_kernels.hip: k_mesh_closest, k_ring_pick) and the surface
// chamfer closure (closure.hip: k_surf_fwd).  Region test of Ericson, Real-Time Collision Detection 5.1.5.
#pragma once
#include <hip/hip_runtime.h>

#ifndef UUO_INF
#define UUO_INF __builtin_huge_valf()
#endif

struct TriHit {
  float cx, cy, cz, d2;
};
__device__ __forceinline__ TriHit closest_on_triangle(float px, float py, float pz, float ax, float ay, float az,
                                                      float bx, float by, float bz, float cx, float cy, float cz) {
  const float abx = bx - ax, aby = by - ay, abz = bz - az;
  const float acx = cx - ax, acy = cy - ay, acz = cz - az;
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float d1 = abx * apx + aby * apy + abz * apz, d2 = acx * apx + acy * apy + acz * apz;
  const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const float d3 = abx * bpx + aby * bpy + abz * bpz, d4 = acx * bpx + acy * bpy + acz * bpz;
  const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const float d5 = abx * cpx + aby * cpy + abz * cpz, d6 = acx * cpx + acy * cpy + acz * cpz;
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  float v, w;  // closest point = a + v*ab + w*ac
  if (d1 <= 0.f && d2 <= 0.f) {  // vertex region a
    v = 0.f; w = 0.f;
  } else if (d3 >= 0.f && d4 <= d3) {  // vertex region b
    v = 1.f; w = 0.f;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {  // edge ab
    v = d1 / (d1 - d3); w = 0.f;
  } else if (d6 >= 0.f && d5 <= d6) {  // vertex region c
    v = 0.f; w = 1.f;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {  // edge ac
    v = 0.f; w = d2 / (d2 - d6);
  } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {  // edge bc
    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.f - w;
  } else {  // interior
    const float denom = 1.f / (va + vb + vc);
    v = vb * denom; w = vc * denom;
  }
  TriHit h;
  h.cx = ax + abx * v + acx * w;
  h.cy = ay + aby * v + acy * w;
  h.cz = az + abz * v + acz * w;
  const float ex = px - h.cx, ey = py - h.cy, ez = pz - h.cz;
  h.d2 = ex * ex + ey * ey + ez * ez;
  if (!(h.d2 == h.d2)) h.d2 = UUO_INF;  // degenerate triangle (0/0): never the winner
  return h;
}

// trimesh.triangles.points_to_barycentric(method="cramer") of a point q in the plane of triangle (a, b, c): the arithmetic of
// k_mesh_closest's epilogue.  A triangle without area (the one-ring's stand-in for a vertex that has no face: a = b = c) has no
// such coordinates; it reports (1, 0, 0).
__device__ __forceinline__ void tri_bary_cramer(float qx, float qy, float qz, float ax, float ay, float az, float bx, float by,
                                                float bz, float cx, float cy, float cz, float* bary) {
  const float e0x = bx - ax, e0y = by - ay, e0z = bz - az, e1x = cx - ax, e1y = cy - ay, e1z = cz - az;
  const float wx = qx - ax, wy = qy - ay, wz = qz - az;
  const float dot00 = e0x * e0x + e0y * e0y + e0z * e0z, dot01 = e0x * e1x + e0y * e1y + e0z * e1z;
  const float dot02 = e0x * wx + e0y * wy + e0z * wz, dot11 = e1x * e1x + e1y * e1y + e1z * e1z;
  const float dot12 = e1x * wx + e1y * wy + e1z * wz;
  const float det = dot00 * dot11 - dot01 * dot01;
  const float inv = 1.f / det;
  const float b2 = (dot00 * dot12 - dot01 * dot02) * inv, b1 = (dot11 * dot02 - dot01 * dot12) * inv;
  const bool ok = det != 0.f && b1 == b1 && b2 == b2;
  bary[0] = ok ? 1.f - b1 - b2 : 1.f;
  bary[1] = ok ? b1 : 0.f;
  bary[2] = ok ? b2 : 0.f;
}
