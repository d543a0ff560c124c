// Forward kernels of the closures' side terms -- floor contact, bone-capsule self-penetration, 2D key-point reprojection,
// joint-angle limits, pose acceleration, the pose prior's per-(frame, joint) weights -- with the setters that configure them on a fit workspace.
// Each kernel leaves upstream gradients and per-frame loss shares for the backward kernels of the same evaluation (closure.hip:
// the temporal instantiations of bwd_body); they share no device code with it but frame_math.h.  closure.hip reaches them
// through uuo_launch_side_terms.
#include <cstring>

#include "frame_math.h"

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_floor): a floor-contact term on K sole vertices (2 <= K <= 16; the left
// foot's K_L points first, s(p) the foot of point p), z up, the plane at height h, contact labels c[F][2] in [0, 1]:
//   pen[t][p] = max(h - z[t][p], 0)                       (always on)
//   flo[t][s] = max(min_{p of foot s} z[t][p] - h, 0)      (the foot's lowest point; the first in list order on ties)
//   loss += w_pen sum pen^2 / (F K) + w_con sum c[t][s] flo[t][s]^2 / (2 F)
//   dL/dz[t][p] = -2 w_pen pen / (F K) + [p = argmin of its foot] w_con c flo / F,   x and y components 0.
// k_floor_fwd: one wave per frame.  It starts from the frame's FrameLds as k_pose_prep (or the closure's forward) left them,
// gathers the K vertices four at a time (one per 16-lane group: the arithmetic of the backward kernel's item loop, in its
// order), evaluates the term on lanes 0 .. K-1 and writes the K upstream gradients and the frame's weighted share of the loss.
// The backward kernels (ACCEL instantiations of bwd_body) take the points as items M .. M + K - 1.
// ----------------------------------------------------------------------------------------------------
struct FloorFwdArgs {
  uuo_gptr<const float> PT, ST, vt, Ww;
  uuo_gptr<const int> Wi;
  int V, F, K, KL;               // K points, the first KL of them on the left foot
  uuo_gptr<const float> frames;  // [F][FrameLds]
  uuo_gptr<const float> trans;   // [F][3] or null
  uuo_gptr<const int> vids;      // [K]
  uuo_gptr<const float> contacts;  // [F][2] or null (ccon == 0)
  float h, cpen, ccon;           // plane height, w_pen / (F K), w_con / (2 F)
  uuo_gptr<float> up;            // [F][K][3] out
  uuo_gptr<float> loss;          // [F] out
};
__global__ __launch_bounds__(64) void k_floor_fwd(FloorFwdArgs a) {
  __shared__ FrameLds L;
  __shared__ float sA[UUO_NUM_JOINTS * 12];
  __shared__ float spf[UUO_KB];
  __shared__ float sz[UUO_FLOOR_MAXK];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int K = a.K;
  {
    constexpr int NW = sizeof(FrameLds) / 4;
    float* dst_l = reinterpret_cast<float*>(&L);
    for (int i = lane; i < NW; i += 64) dst_l[i] = a.frames[(size_t)f * NW + i];
  }
  __syncthreads();
  if (lane < UUO_NUM_JOINTS) frame_skin_matrix(L, lane, sA + lane * 12);
  for (int i = lane; i < UUO_KB; i += 64) {
    float v = 0.f;
    if (i < UUO_NUM_POSE_FEATS) {
      const int j = 1 + i / 9, e = i % 9;
      v = L.R[j][e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
    spf[i] = v;
  }
  __syncthreads();
  const float trz = a.trans ? a.trans[(size_t)f * 3 + 2] : 0.f;
  const int gq = lane >> 4, sl = lane & 15;
  float fk[13];
#pragma unroll
  for (int t = 0; t < 13; ++t) fk[t] = spf[sl + 16 * t];
  const float beta_s = (sl < 10) ? L.beta[sl] : 0.f;
  auto row_sum = [](float v) {
    v += dpp_rot<0x128>(v);
    v += dpp_rot<0x124>(v);
    v += dpp_rot<0x122>(v);
    v += dpp_rot<0x121>(v);
    return v;
  };
  for (int r = 0; r < (K + 3) / 4; ++r) {
    const int p = gq + 4 * r;
    int vi = (p < K) ? a.vids[p] : 0;
    if ((unsigned)vi >= (unsigned)a.V) vi = 0;  // (uuo_fit_set_floor has checked the ids; keeps the gather in bounds)
    const float* pt = a.PT + (size_t)vi * 3 * UUO_KB + sl;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 13; ++t) {
      s0 = fmaf(pt[16 * t], fk[t], s0);
      s1 = fmaf(pt[UUO_KB + 16 * t], fk[t], s1);
      s2 = fmaf(pt[2 * UUO_KB + 16 * t], fk[t], s2);
    }
    const float* ps = a.ST + (size_t)vi * 30 + (sl < 10 ? sl : 0);
    const float st0 = (sl < 10) ? ps[0] : 0.f, st1 = (sl < 10) ? ps[10] : 0.f, st2 = (sl < 10) ? ps[20] : 0.f;
    float vp[3];
    vp[0] = row_sum(s0) + (a.vt[(size_t)vi * 3] + row_sum(st0 * beta_s));
    vp[1] = row_sum(s1) + (a.vt[(size_t)vi * 3 + 1] + row_sum(st1 * beta_s));
    vp[2] = row_sum(s2) + (a.vt[(size_t)vi * 3 + 2] + row_sum(st2 * beta_s));
    const int4 wi = *reinterpret_cast<const int4*>(a.Wi + (size_t)vi * 4);
    const float4 w4 = *reinterpret_cast<const float4*>(a.Ww + (size_t)vi * 4);
    const int wj[4] = {wi.x, wi.y, wi.z, wi.w};
    const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
    float T8 = 0.f, T9 = 0.f, T10 = 0.f, T11 = 0.f;  // the z row of the blended transform
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const float4 r2 = reinterpret_cast<const float4*>(sA + wj[n] * 12)[2];
      T8 = fmaf(ww[n], r2.x, T8); T9 = fmaf(ww[n], r2.y, T9); T10 = fmaf(ww[n], r2.z, T10); T11 = fmaf(ww[n], r2.w, T11);
    }
    const float vz = fmaf(T10, vp[2], fmaf(T9, vp[1], T8 * vp[0])) + T11 + trz;
    if (p < K && sl == 0) sz[p] = vz;
  }
  __syncthreads();
  const float c0 = (a.ccon != 0.f) ? a.contacts[(size_t)f * 2] : 0.f, c1 = (a.ccon != 0.f) ? a.contacts[(size_t)f * 2 + 1] : 0.f;
  if (lane < K) {
    const int p = lane, foot = (p < a.KL) ? 0 : 1;
    const int lo = foot ? a.KL : 0, hi = foot ? K : a.KL;
    int am = lo;
    float zm = sz[lo];
    for (int q = lo + 1; q < hi; ++q) {
      const float zq = sz[q];
      if (zq < zm) {
        zm = zq;
        am = q;
      }
    }
    const float pen = fmaxf(a.h - sz[p], 0.f), flo = fmaxf(zm - a.h, 0.f), c = foot ? c1 : c0;
    float dz = -2.f * a.cpen * pen;
    if (p == am) dz += 2.f * a.ccon * c * flo;
    float* pu = a.up + ((size_t)f * K + p) * 3;
    pu[0] = 0.f;
    pu[1] = 0.f;
    pu[2] = dz;
  }
  if (lane == 0) {  // the frame's share, in a fixed order
    float sp = 0.f, zl = sz[0], zr = sz[a.KL];
    for (int p = 0; p < K; ++p) {
      const float pen = fmaxf(a.h - sz[p], 0.f);
      sp += pen * pen;
      if (p < a.KL) zl = fminf(zl, sz[p]);
      else zr = fminf(zr, sz[p]);
    }
    const float fl0 = fmaxf(zl - a.h, 0.f), fl1 = fmaxf(zr - a.h, 0.f);
    a.loss[f] = a.cpen * sp + a.ccon * (c0 * (fl0 * fl0) + c1 * (fl1 * fl1));
  }
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_capsules): a bone-capsule self-penetration term.  Capsule c = (u, v, alpha,
// beta, r): end points a = J_u + alpha (J_v - J_u), b = J_u + beta (J_v - J_u) on the line through two world joints J = G_j^t
// (no translation: the term is translation invariant), radius r.  For every pair k = (i, j) of the list:
//   (s, t) = closest-point parameters of the segments [a_i, b_i], [a_j, b_j] (Ericson, Real-Time Collision Detection 5.1.9;
//            capsule_closest below, degenerate when |d|^2 <= 1e-12, parallel when den <= 1e-6 A E)
//   delta = c_i - c_j,  d = |delta|,  pen = max(r_i + r_j - d, 0),  loss += w pen^2 / F,
//   dL/dc_i = -(2 w / F) pen delta / d = -dL/dc_j   (s, t held fixed: envelope theorem; d = 0: no gradient, pen^2 still counts)
//   gamma_i = alpha_i + s (beta_i - alpha_i):  dL/dJ_{u_i} += (1 - gamma_i) dL/dc_i,  dL/dJ_{v_i} += gamma_i dL/dc_i  (same for j).
// k_capsule_fwd: one wave per frame.  It reads the 24 G^t of the frame's FrameLds (as the closure's forward or k_pose_prep left
// them), forms the <= 32 capsules' end points in LDS, evaluates the <= 256 pairs (pair k on lane k % 64, up to four per lane) and
// parks the four end joints' shares of each pair's gradient -- (1 - gamma_i) dL/dc_i, gamma_i dL/dc_i, -(1 - gamma_j) dL/dc_i,
// -gamma_j dL/dc_i -- in LDS.  The 72 (joint, component) outputs -- lanes 0..63, then lanes 0..7 once more -- are summed over the
// joint's rows of the host-built CSR table, which lists (pair, end) in pair order and, inside a pair, in the order u_i, v_i, u_j,
// v_j.  The frame's sum of pen^2: every lane adds its own pairs in order, then a fixed xor butterfly (32, 16, .. 1) adds the
// lanes.  The table and the geometry are fetched into LDS once, beside G^t: one global round trip.  No atomics: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
#define UUO_CAPS_MAXC 32
#define UUO_CAPS_MAXP 256
#define UUO_CAPS_TAB_PAIRS (UUO_CAPS_MAXC * 2)                       // cap_tab layout (ints): joints, pairs, CSR offsets, CSR entries
#define UUO_CAPS_TAB_OFF (UUO_CAPS_TAB_PAIRS + UUO_CAPS_MAXP * 2)
#define UUO_CAPS_TAB_ENT (UUO_CAPS_TAB_OFF + UUO_NUM_JOINTS + 1)
#define UUO_CAPS_TAB_INTS (UUO_CAPS_TAB_ENT + UUO_CAPS_MAXP * 4)
struct CapsFwdArgs {
  uuo_gptr<const float> frames;  // [F][FrameLds]
  uuo_gptr<const int> tab;       // the workspace's table (layout above)
  uuo_gptr<const float> geom;    // [C][3] alpha, beta, radius
  int C, P;
  float cl, cg;                  // w / F, 2 w / F
  uuo_gptr<float> up;            // [F][24][3] out
  uuo_gptr<float> loss;          // [F] out
};
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
// closest-point parameters of the segments p1 + s d1, p2 + t d2 (s, t in [0, 1]); r = p1 - p2
struct CapsVec { float x, y, z; };
__device__ __forceinline__ float caps_dot(CapsVec a, CapsVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float2 capsule_closest(CapsVec d1, CapsVec d2, CapsVec r) {
  const float A = caps_dot(d1, d1), E = caps_dot(d2, d2);
  const float fq = caps_dot(d2, r), cq = caps_dot(d1, r), bq = caps_dot(d1, d2);
  const bool dA = A <= 1e-12f, dE = E <= 1e-12f;
  if (dA && dE) return make_float2(0.f, 0.f);
  if (dA) return make_float2(0.f, clamp01(fq / E));
  if (dE) return make_float2(clamp01(-cq / A), 0.f);
  const float den = A * E - bq * bq;
  float s = (den > 1e-6f * (A * E)) ? clamp01((bq * fq - cq * E) / den) : 0.f;
  float t = (bq * s + fq) / E;
  if (t < 0.f) {
    t = 0.f;
    s = clamp01(-cq / A);
  } else if (t > 1.f) {
    t = 1.f;
    s = clamp01((bq - cq) / A);
  }
  return make_float2(s, t);
}
__global__ __launch_bounds__(64) void k_capsule_fwd(CapsFwdArgs a) {
  __shared__ float sG[UUO_NUM_JOINTS * 3];
  __shared__ int sTab[UUO_CAPS_TAB_INTS];           // the workspace's table: one coalesced fetch, every lookup below is LDS
  __shared__ float sGeom[UUO_CAPS_MAXC * 3];
  __shared__ float sEnd[UUO_CAPS_MAXC][6];          // a, b of every capsule
  __shared__ float sCon[UUO_CAPS_MAXP * 4][3];      // per (pair, end): that end joint's share of dL/dc, signed
  const int f = blockIdx.x, lane = threadIdx.x;
  const int C = min(a.C, UUO_CAPS_MAXC), P = min(a.P, UUO_CAPS_MAXP);  // (uuo_fit_set_capsules has checked them; keeps LDS in bounds)
  {
    constexpr int NW = sizeof(FrameLds) / 4, GT = offsetof(FrameLds, Gt) / 4;
    for (int i = lane; i < UUO_NUM_JOINTS * 3; i += 64) sG[i] = a.frames[(size_t)f * NW + GT + i];
    for (int i = lane; i < UUO_CAPS_TAB_INTS; i += 64) sTab[i] = a.tab[i];
    for (int i = lane; i < UUO_CAPS_MAXC * 3; i += 64) sGeom[i] = a.geom[i];
  }
  __syncthreads();
  if (lane < C) {
    const int u = sTab[lane * 2] % UUO_NUM_JOINTS, v = sTab[lane * 2 + 1] % UUO_NUM_JOINTS;
    const float al = sGeom[lane * 3], be = sGeom[lane * 3 + 1];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float ju = sG[u * 3 + c], e = sG[v * 3 + c] - ju;
      sEnd[lane][c] = ju + al * e;
      sEnd[lane][3 + c] = ju + be * e;
    }
  }
  __syncthreads();
  float part = 0.f;  // this lane's pen^2, pairs lane, lane + 64, ... in that order
  for (int k = lane; k < P; k += 64) {
    const int i = sTab[UUO_CAPS_TAB_PAIRS + k * 2] % UUO_CAPS_MAXC, j = sTab[UUO_CAPS_TAB_PAIRS + k * 2 + 1] % UUO_CAPS_MAXC;
    const CapsVec p1 = {sEnd[i][0], sEnd[i][1], sEnd[i][2]}, p2 = {sEnd[j][0], sEnd[j][1], sEnd[j][2]};
    const CapsVec d1 = {sEnd[i][3] - p1.x, sEnd[i][4] - p1.y, sEnd[i][5] - p1.z};
    const CapsVec d2 = {sEnd[j][3] - p2.x, sEnd[j][4] - p2.y, sEnd[j][5] - p2.z};
    const CapsVec r = {p1.x - p2.x, p1.y - p2.y, p1.z - p2.z};
    const float2 st = capsule_closest(d1, d2, r);
    const float s = st.x, t = st.y;
    const CapsVec dl = {(p1.x + s * d1.x) - (p2.x + t * d2.x), (p1.y + s * d1.y) - (p2.y + t * d2.y), (p1.z + s * d1.z) - (p2.z + t * d2.z)};
    const float d = sqrtf(caps_dot(dl, dl));
    const float pen = fmaxf((sGeom[i * 3 + 2] + sGeom[j * 3 + 2]) - d, 0.f);
    const float q = (d > 0.f) ? -(a.cg * pen) / d : 0.f;
    const float g[3] = {q * dl.x, q * dl.y, q * dl.z};  // dL/dc_i = -dL/dc_j
    const float ai = sGeom[i * 3], aj = sGeom[j * 3];
    const float gi = ai + s * (sGeom[i * 3 + 1] - ai), gj = aj + t * (sGeom[j * 3 + 1] - aj);
    const float co[4] = {1.f - gi, gi, 1.f - gj, gj};   // ends u_i, v_i, u_j, v_j
#pragma unroll
    for (int end = 0; end < 4; ++end)
#pragma unroll
      for (int c = 0; c < 3; ++c) sCon[k * 4 + end][c] = co[end] * ((end & 2) ? -g[c] : g[c]);
    part += pen * pen;
  }
  __syncthreads();
  for (int o = lane; o < UUO_NUM_JOINTS * 3; o += 64) {
    const int jj = o / 3, c = o - jj * 3;
    const int e0 = max(sTab[UUO_CAPS_TAB_OFF + jj], 0), e1 = min(sTab[UUO_CAPS_TAB_OFF + jj + 1], 4 * P);
    float acc = 0.f;
    for (int e = e0; e < e1; e += 4) {  // four rows a step: the LDS reads overlap, the adds keep the rows' (= the pairs') order
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ent = (e + u < e1) ? sTab[UUO_CAPS_TAB_ENT + e + u] : -1;
        v[u] = (ent >= 0) ? sCon[ent % (UUO_CAPS_MAXP * 4)][c] : 0.f;
      }
      acc = (((acc + v[0]) + v[1]) + v[2]) + v[3];
    }
    a.up[(size_t)f * 72 + o] = acc;
  }
  // the frame's share: the lanes' partial sums (each in pair order) through a fixed butterfly, lane l with lane l ^ 32, 16, .. 1
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  if (lane == 0) a.loss[f] = a.cl * part;
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_joint_limits): a joint-angle limit term on the body pose.  Body joint
// j = 1 .. 23, R its local rotation as frame_forward forms it (gs6d_forward of the raw entries when the stage normalises, the raw
// entries otherwise: the same function on the same inputs, so R is bit for bit the forward's), row-major:
//   s = 1/2 (R21 - R12, R02 - R20, R10 - R01),  c = 1/2 (R00 + R11 + R22 - 1),  n = |s|,  theta = atan2(n, c),  kappa = theta / n,
//   omega = kappa s;   n < 1e-4: c >= 0 takes kappa = 1, d kappa = 0 (identity), c < 0 contributes nothing (half turn: no axis)
//   pen_k = max(omega_k - hi_k, 0) + max(lo_k - omega_k, 0),  loss += w pen_k^2 / F,
//   g_k = dL/d omega_k = (2 w / F) (max(omega_k - hi_k, 0) - max(lo_k - omega_k, 0)),  q = s . g,
//   dL/ds = kappa g + q (d kappa / dn) s / n,  dL/dc = q d kappa / dc,
//   d kappa / dn = c / (n (n^2 + c^2)) - theta / n^2,  d kappa / dc = -1 / (n^2 + c^2),
//   dL/dR21 += 1/2 dL/ds_x, dL/dR12 -= 1/2 dL/ds_x, ... (cyclic),  dL/dR_kk += 1/2 dL/dc.
// k_limit_fwd: 32 lanes per frame, two frames per 64-thread block (a frame has 23 joints: a wave per frame would leave 41 lanes
// idle; F odd leaves the last block's upper half idle).  Lane l < 23 of a half takes joint l + 1: raw entries and the six bounds
// in one round trip, R, omega, the hinges, dL/dR, and the stage's normalisation backward (gs6d_backward) on its own raw entries:
// it writes the gradient in PARAMETER space, [F][23][9], third rows exact zeros when the stage normalises.  The frame's 69
// squares: every lane adds its three in the order x, y, z, then a fixed xor butterfly (16, 8, .. 1) inside the half adds the
// lanes (lanes 23 .. 31 hold zeros).  No atomics, no LDS: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
#define UUO_LIM_FPB 2  // frames per block
struct LimitFwdArgs {
  uuo_gptr<const float> body;  // [F][23][9] raw body pose entries (UuoPoseSrc.body)
  uuo_gptr<const float> tab;   // [2][23][3] lo, hi
  int F, norm_body;
  float cl, cg;                // w / F, 2 w / F
  uuo_gptr<float> g;           // [F][23][9] out
  uuo_gptr<float> loss;        // [F] out
};
__global__ __launch_bounds__(64) void k_limit_fwd(LimitFwdArgs a) {
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int f = blockIdx.x * UUO_LIM_FPB + half;
  const bool on = f < a.F && l < 23;
  float raw[9], lo[3], hi[3];
#pragma unroll
  for (int e = 0; e < 9; ++e) raw[e] = on ? a.body[((size_t)f * 23 + l) * 9 + e] : ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = on ? a.tab[l * 3 + k] : -INFINITY;
    hi[k] = on ? a.tab[69 + l * 3 + k] : INFINITY;
  }
  float R[9];
  if (a.norm_body) {
    gs6d_forward(raw, R);
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = raw[e];
  }
  const float s[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
  const float c = 0.5f * (((R[0] + R[4]) + R[8]) - 1.f);
  const float n2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
  const float n = sqrtf(n2);
  const bool small = n < 1e-4f;
  const bool skip = small && c < 0.f;
  const float nn = small ? 1.f : n;  // (keeps the quotients of the unused branch finite)
  const float theta = atan2f(n, c);
  const float kappa = small ? 1.f : theta / nn;
  const float den = small ? 1.f : n2 + c * c;
  const float dkn = small ? 0.f : (c / (nn * den) - theta / (nn * nn));
  const float dkc = small ? 0.f : (-1.f / den);
  float g[3], part = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float om = kappa * s[k];
    const float up = fmaxf(om - hi[k], 0.f), dn = fmaxf(lo[k] - om, 0.f);
    const float pen = (skip || !on) ? 0.f : up + dn;
    g[k] = (skip || !on) ? 0.f : a.cg * (up - dn);
    part += pen * pen;
  }
  const float q = (s[0] * g[0] + s[1] * g[1]) + s[2] * g[2];
  const float qn = q * dkn / nn;
  const float ds[3] = {0.5f * (kappa * g[0] + qn * s[0]), 0.5f * (kappa * g[1] + qn * s[1]), 0.5f * (kappa * g[2] + qn * s[2])};
  const float dc = 0.5f * (q * dkc);
  const float dR[9] = {dc, -ds[2], ds[1], ds[2], dc, -ds[0], -ds[1], ds[0], dc};
  float out[9];
  if (a.norm_body) {
    float da[6];
    gs6d_backward(raw, dR, da);
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = da[e];
    out[6] = out[7] = out[8] = 0.f;
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = dR[e];
  }
  if (on) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.g[((size_t)f * 23 + l) * 9 + e] = out[e];
  }
  // the frame's share: the lanes' sums (each x, y, z in order) through a fixed butterfly inside the 32-lane half
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  if (l == 0 && f < a.F) a.loss[f] = a.cl * part;
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_pose_gmm): SMPLify's max-mixture pose prior on the body pose.  theta [69] is
// the concatenation of the body joints' axis-angle vectors omega_j, each formed as k_limit_fwd forms it (same R, same branches;
// a half turn gives omega_j = 0 and receives no gradient).  Component k = 0 .. K-1 (K <= 16): mean mu_k, A_k lower triangular with
// A_k A_k^T the inverse covariance, offset b_k >= 0:
//   y_k = A_k^T (theta - mu_k),  e_k = 1/2 |y_k|^2 + b_k,  k* = argmin_k e_k (ties: the lowest k),  loss += (w / F) e_k*,
//   dL/d theta = (w / F) A_k* y_k*            (no gradient through the choice),
// then k_limit_fwd's chain per joint (dL/ds, dL/dc -> dL/dR -> gs6d_backward) into PARAMETER space.
// k_pose_gmm delivers gradients and shares through the buffer of the joint-angle limit term with the protocol of k_prior_conf:
// add == 0 writes the buffer, add != 0 (k_limit_fwd of this evaluation ran before it on the same stream) adds to it.
// A block of 512 threads (eight waves) takes UUO_GMM_FPB = 8 frames and reads every table entry of step 1 once for all of them:
//   0. thread (slot = t / 32, l = t % 32 < 23), t < 256 (four of the eight waves: 32 lanes a frame), forms omega of joint l + 1 of its frame and keeps raw, s,
//      kappa and the two derivatives in registers for step 4; theta goes to LDS, frame minor.  A slot past F holds theta = 0 and
//      stores nothing.
//   1. wave w takes the components k = w, w + 8; lane c holds column c of y_k for the eight frames (lanes 0 .. 4 also columns
//      64 .. 68): y_k[c] = sum_{r = c .. 68} A_k[r][c] (theta[r] - mu_k[r]), r ascending -- one coalesced row of the packed
//      triangle per step, used by all eight frames, seven rows fetched at a time.  |y_k|^2: lane c adds y[c]^2 and y[64 + c]^2,
//      then a fixed xor butterfly (32, 16, .. 1).  The wave keeps the best (e, k, y) per frame in registers (strict <: the
//      lowest k of the wave stays).
//   2. the eight waves' bests meet in LDS: the least e, on ties the lowest k; the winner's wave parks its y in LDS.
//   3. wave w takes frame w: lane r forms row r of A_k* y (lanes 0 .. 4 also rows 64 .. 68), c ascending, seven entries of the
//      row fetched at a time.
//   4. thread (slot, l) runs the chain on its joint's three entries and writes or adds its nine gradients; lane 0 of a slot the
//      frame's share and the winner (gmm_win: F ints that only the checkers read, see uuo_fit_set_pose_gmm).
// Every sum's order is fixed by (r, c, lane) alone: it depends neither on the grid nor on F nor on the other frames of the block.
// No atomics, 7 KB of LDS, no scratch: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
#define UUO_GMM_FPB 8  // frames per block
struct PoseGmmArgs {
  uuo_gptr<const float> body;  // [F][23][9] raw body pose entries (UuoPoseSrc.body)
  uuo_gptr<const float> tab;   // the workspace's table (uuo_common.h: UUO_GMM_TAB_*)
  int F, K, norm_body, add;
  float cw;                    // w / F
  uuo_gptr<float> g;           // [F][23][9] gradients, then [F] shares: written (add == 0) or added to
  uuo_gptr<int32_t> win;       // [F] out: the winning component (null: not stored)
};
#define UUO_GMM_WAVES 8  // waves per block: one frame each in step 3
#define UUO_GMM_PF 7     // table entries a lane has in flight (7: 155 VGPRs; 8 takes 164, past the 160 of the kernels beside it)
__global__ __launch_bounds__(64 * UUO_GMM_WAVES) void k_pose_gmm(PoseGmmArgs a) {
  constexpr int FPB = UUO_GMM_FPB;
  __shared__ __attribute__((aligned(16))) float sTh[69][FPB];  // theta, frame minor
  __shared__ float sY[FPB][72], sG[FPB][72];                   // the winner's y, then (w / F) A y
  constexpr int NW = UUO_GMM_WAVES, PF = UUO_GMM_PF;
  static_assert(NW == FPB, "step 3 gives every wave one frame");
  __shared__ float sBe[NW][FPB], sE[FPB];
  __shared__ int sBk[NW][FPB], sK[FPB];
  const int t = threadIdx.x, slot = (t >> 5) & (FPB - 1), l = t & 31;  // (steps 0 and 4 run on t < 256: 32 lanes a frame)
  const int f = blockIdx.x * FPB + slot;
  const bool on = t < 32 * FPB && f < a.F && l < 23;
  const int K = min(max(a.K, 1), UUO_GMM_MAXK);  // (uuo_fit_set_pose_gmm has checked it; keeps the table reads in bounds)
  const size_t row = on ? ((size_t)f * 23 + l) * 9 : 0;
  // 0. omega of this thread's joint, as k_limit_fwd
  float raw[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) raw[e] = on ? a.body[row + e] : ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
  float R[9];
  if (a.norm_body) {
    gs6d_forward(raw, R);
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = raw[e];
  }
  const float s[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
  const float c = 0.5f * (((R[0] + R[4]) + R[8]) - 1.f);
  const float n2 = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
  const float n = sqrtf(n2);
  const bool small = n < 1e-4f;
  const bool skip = small && c < 0.f;
  const float nn = small ? 1.f : n;  // (keeps the quotients of the unused branch finite)
  const float theta = atan2f(n, c);
  const float kappa = small ? 1.f : theta / nn;
  const float den = small ? 1.f : n2 + c * c;
  const float dkn = small ? 0.f : (c / (nn * den) - theta / (nn * nn));
  const float dkc = small ? 0.f : (-1.f / den);
  if (t < 32 * FPB && l < 23) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sTh[3 * l + k][slot] = (skip || !on) ? 0.f : kappa * s[k];
  }
  __syncthreads();
  // 1. y_k and e_k of this wave's components, for the block's frames
  const int w = t >> 6, ln = t & 63;
  const bool tail = ln < 5;           // this lane also holds column (step 3: row) 64 + ln
  const int c2 = tail ? 64 + ln : 0;
  float be[FPB], by[FPB], by2[FPB];
  int bk[FPB];
#pragma unroll
  for (int i = 0; i < FPB; ++i) {
    be[i] = INFINITY;
    by[i] = by2[i] = 0.f;
    bk[i] = UUO_GMM_MAXK;
  }
  for (int k = w; k < K; k += NW) {
    const float* A = a.tab + (size_t)k * UUO_GMM_TRI;
    const float* mu = a.tab + UUO_GMM_TAB_MEANS + k * 69;
    const float off = a.tab[UUO_GMM_TAB_OFFS + k];
    float acc[FPB], acc2[FPB];
#pragma unroll
    for (int i = 0; i < FPB; ++i) acc[i] = acc2[i] = 0.f;
    // rows in batches of PF: a batch's entries and means are fetched together (one round trip a batch, not one a row: the
    // kernel's time is the table's trip from L2), then applied row by row -- the order of every sum stays r ascending
#pragma unroll 1
    for (int rb = 0; rb < 69; rb += PF) {
      float av[PF], mv[PF];
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int r = min(rb + u, 68);
        av[u] = A[r * (r + 1) / 2 + min(ln, r)];
        mv[u] = mu[r];
      }
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int r = min(rb + u, 68);
        const bool act = rb + u < 69 && ln <= r;
        const float4 t0 = *reinterpret_cast<const float4*>(&sTh[r][0]), t1 = *reinterpret_cast<const float4*>(&sTh[r][4]);
        const float th[FPB] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
        for (int i = 0; i < FPB; ++i) acc[i] = act ? fmaf(av[u], th[i] - mv[u], acc[i]) : acc[i];
        __builtin_amdgcn_sched_barrier(0);  // (keeps the next rows' LDS reads behind this row: eight more VGPRs a row otherwise)
      }
    }
#pragma unroll
    for (int r = 64; r < 69; ++r) {  // columns 64 .. 68 on lanes 0 .. 4
      const bool act = tail && c2 <= r;
      const float av = A[r * (r + 1) / 2 + (act ? c2 : 0)];
      const float m = mu[r];
      const float4 t0 = *reinterpret_cast<const float4*>(&sTh[r][0]), t1 = *reinterpret_cast<const float4*>(&sTh[r][4]);
      const float th[FPB] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
      for (int i = 0; i < FPB; ++i) acc2[i] = act ? fmaf(av, th[i] - m, acc2[i]) : acc2[i];
    }
#pragma unroll
    for (int i = 0; i < FPB; ++i) {
      float sq = fmaf(acc2[i], acc2[i], acc[i] * acc[i]);
#pragma unroll
      for (int mk = 32; mk >= 1; mk >>= 1) sq += __shfl_xor(sq, mk, 64);
      const float e = fmaf(0.5f, sq, off);
      if (e < be[i]) {
        be[i] = e;
        bk[i] = k;
        by[i] = acc[i];
        by2[i] = acc2[i];
      }
    }
  }
  // 2. the winner of every frame over the block's eight waves: the least e, on ties the lowest k
  if (ln == 0) {
#pragma unroll
    for (int i = 0; i < FPB; ++i) {
      sBe[w][i] = be[i];
      sBk[w][i] = bk[i];
    }
  }
  __syncthreads();
  if (t < FPB) {
    float e0 = sBe[0][t];
    int k0 = sBk[0][t];
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      const float e = sBe[q][t];
      const int kq = sBk[q][t];
      if (e < e0 || (e == e0 && kq < k0)) {
        e0 = e;
        k0 = kq;
      }
    }
    sE[t] = e0;
    sK[t] = min(k0, K - 1);  // (k0 = 16 only when no e_k compared at all, a NaN pose: keeps the reads below in bounds)
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < FPB; ++i) {
    if (w == (sK[i] & (NW - 1))) {  // (component k is wave k % 8's)
      sY[i][ln] = by[i];
      if (tail) sY[i][c2] = by2[i];
    }
  }
  __syncthreads();
  // 3. (w / F) A_k* y: rows ln and 64 + ln of frame w, the row's entries in batches of PF as above
  {
    const int i = w;
    const float* A = a.tab + (size_t)sK[i] * UUO_GMM_TRI;
    const int base1 = ln * (ln + 1) / 2, base2 = c2 * (c2 + 1) / 2;
    float g1 = 0.f, g2 = 0.f;
#pragma unroll 1
    for (int cb = 0; cb < 69; cb += PF) {
      float a1[PF], a2[PF];
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        a1[u] = A[base1 + min(cb + u, ln)];
        a2[u] = A[base2 + min(cb + u, c2)];
      }
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int cc = cb + u;
        const float y = sY[i][min(cc, 68)];
        g1 = (cc <= ln) ? fmaf(a1[u], y, g1) : g1;
        g2 = (tail && cc <= c2) ? fmaf(a2[u], y, g2) : g2;
      }
    }
    sG[i][ln] = a.cw * g1;
    if (tail) sG[i][c2] = a.cw * g2;
  }
  __syncthreads();
  // 4. k_limit_fwd's chain on this thread's joint
  float g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = (skip || !on) ? 0.f : sG[slot][3 * min(l, 22) + k];
  float old[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) old[e] = (on && a.add) ? a.g[row + e] : 0.f;
  const bool head = t < 32 * FPB && l == 0 && f < a.F;
  const float old_share = (head && a.add) ? a.g[(size_t)a.F * 207 + f] : 0.f;
  const float q = (s[0] * g[0] + s[1] * g[1]) + s[2] * g[2];
  const float qn = q * dkn / nn;
  const float ds[3] = {0.5f * (kappa * g[0] + qn * s[0]), 0.5f * (kappa * g[1] + qn * s[1]), 0.5f * (kappa * g[2] + qn * s[2])};
  const float dc = 0.5f * (q * dkc);
  const float dR[9] = {dc, -ds[2], ds[1], ds[2], dc, -ds[0], -ds[1], ds[0], dc};
  float out[9];
  if (a.norm_body) {
    float da[6];
    gs6d_backward(raw, dR, da);
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = old[e] + da[e];
    out[6] = old[6]; out[7] = old[7]; out[8] = old[8];
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = old[e] + dR[e];
  }
  if (on) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.g[row + e] = out[e];
  }
  if (head) {
    a.g[(size_t)a.F * 207 + f] = old_share + a.cw * sE[slot];
    if (a.win) a.win[f] = sK[slot];
  }
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_prior_weights): the pose prior of the chamfer and marker stages with a weight
// per (frame, body joint), w[t][j] >= 0:
//   loss += c sum_t sum_j w[t][j] sum_e (raw[t][j][e] - o[t][j][e])^2,   c = w_pose / (F 207)   (the normaliser of the uniform
//   prior, not sum w: w == 1 everywhere is the uniform term),   dL/d raw[t][j][e] = 2 c w[t][j] (raw - o).
// k_prior_conf delivers the WHOLE prior -- the backward kernels and the finalize then run with a pose coefficient of 0 -- through
// the buffer of the joint-angle limit term, [F][23][9] gradients in parameter space and [F] shares behind them, which the
// temporal instantiations add to gout and to slot 3 (lim_g != null): no existing kernel changes.  add == 0: it writes the buffer;
// add != 0 (the limit term is on, k_limit_fwd of this evaluation ran before it on the same stream): it adds to it.
// The shape of k_limit_fwd: 32 lanes per frame, two frames per 64-thread block.  Lane l < 23 of a half takes joint l + 1: its
// nine raw entries, nine targets, its weight (and with add its nine old gradients; lane 0 the old share) in one round trip -- the
// 23 lanes of a half read 207 consecutive floats of each table.  A weight of 0 stores exact +0 (not 0 * diff), a row on its
// target 2 c w * 0 = 0: third rows on their targets stay exact zeros, as the compact packing needs.  The frame's share: every lane
// sums its nine squares in the order e = 0 .. 8 and weighs the sum, then a fixed xor butterfly (16, 8, .. 1) inside the half adds
// the lanes (lanes 23 .. 31 hold zeros).  No atomics, no LDS: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
struct PriorConfArgs {
  uuo_gptr<const float> body;    // [F][23][9] raw body pose entries (the optimised parameters)
  uuo_gptr<const float> target;  // [F][23][9] the prior's target (uuo_problem_t.d_o_pose)
  uuo_gptr<const float> w;       // [F][23] weights
  int F, add;
  float cl, cg;                  // w_pose / (F 207), 2 w_pose / (F 207)
  uuo_gptr<float> g;             // [F][23][9] gradients, then [F] shares: written (add == 0) or added to
};
__global__ __launch_bounds__(64) void k_prior_conf(PriorConfArgs a) {
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int f = blockIdx.x * UUO_LIM_FPB + half;
  const bool on = f < a.F && l < 23;
  const size_t row = on ? ((size_t)f * 23 + l) * 9 : 0;
  float raw[9], tg[9], old[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    raw[e] = on ? a.body[row + e] : 0.f;
    tg[e] = on ? a.target[row + e] : 0.f;
    old[e] = (on && a.add) ? a.g[row + e] : 0.f;
  }
  const float w = on ? a.w[(size_t)f * 23 + l] : 0.f;
  const bool head = l == 0 && f < a.F;
  const float old_share = (head && a.add) ? a.g[(size_t)a.F * 207 + f] : 0.f;
  const float wc = a.cg * w;
  float sq = 0.f, out[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float diff = raw[e] - tg[e];
    out[e] = old[e] + ((w == 0.f) ? 0.f : wc * diff);
    sq = fmaf(diff, diff, sq);
  }
  if (on) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.g[row + e] = out[e];
  }
  float part = (w == 0.f) ? 0.f : w * sq;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  if (head) a.g[(size_t)a.F * 207 + f] = old_share + a.cl * part;
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_pose_accel): the pose-acceleration term on the local body rotations
// (losses.pose_accel_loss).  Body joint j = 1 .. 23, R_t[j] its local rotation in frame t as k_limit_fwd forms it (gs6d_forward of
// the raw entries when the stage normalises, the raw entries otherwise), u[23] >= 0 joint weights, F >= 3:
//   a_t[j] = R_t[j] - 2 R_{t+1}[j] + R_{t+2}[j]                       t = 0 .. F-3
//   loss += cl sum_t sum_j u[j] |a_t[j]|_F^2                           cl = w / ((F - 2) 207)
//   dL/dR_s[j] = cg u[j] (a_s - 2 a_{s-1} + a_{s-2})                   cg = 2 w / ((F - 2) 207);  a_t outside 0 .. F-3 is 0
// k_pose_accel delivers the gradients in PARAMETER space (gs6d_backward on the lane's own raw entries; third rows exact zeros
// when the stage normalises) and the frames' shares -- frame t holds cl sum_j u[j] |a_t[j]|^2, frames F-2 and F-1 hold 0 --
// through the buffer of the joint-angle limit term with the protocol of k_prior_conf: add == 0 writes the buffer, add != 0
// (k_limit_fwd of this evaluation ran before it on the same stream) adds to it; k_prior_conf, when on, runs after it with add.
// The shape of k_limit_fwd: 32 lanes per frame, two frames per 64-thread block; lane l < 23 of a half takes joint l + 1 of frame
// s.  It loads the joint's raw entries of the five frames s-2 .. s+2, every index clamped to 0 .. F-1 and every load
// unconditional (an idle lane loads a clamped row too), forms the five R and the three a_s, a_{s-1}, a_{s-2}, each SELECTED to
// zero when its t is outside 0 .. F-3.  All loops are unrolled over constants: no private array is indexed dynamically, no
// scratch.  A lane reads no row of the buffer but its own, and that one only with add; every active lane stores all nine entries
// at every evaluation.  A joint weight of 0 leaves the lane's old entries as they are (exact +0 without add).  The frame's
// share: every lane sums the nine squares of a_s in the order e = 0 .. 8 and weighs the sum by u, then a fixed xor butterfly
// (16, 8, .. 1) inside the half adds the lanes (lanes 23 .. 31 hold zeros).  No atomics, no LDS: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
struct PoseAccelArgs {
  uuo_gptr<const float> body;  // [F][23][9] raw body pose entries (UuoPoseSrc.body)
  uuo_gptr<const float> u;     // [23] joint weights
  int F, norm_body, add;
  float cl, cg;                // w / ((F - 2) 207), 2 w / ((F - 2) 207)
  uuo_gptr<float> g;           // [F][23][9] gradients, then [F] shares: written (add == 0) or added to
};
__global__ __launch_bounds__(64) void k_pose_accel(PoseAccelArgs a) {
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int f = blockIdx.x * UUO_LIM_FPB + half;
  const bool on = f < a.F && l < 23;
  const int s = min(f, a.F - 1), jl = min(l, 22);  // (an idle lane computes on a clamped row and stores nothing)
  const size_t row = ((size_t)s * 23 + jl) * 9;
  float raw[5][9], R[5][9], old[9];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const size_t rk = ((size_t)min(max(s + k - 2, 0), a.F - 1) * 23 + jl) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) raw[k][e] = a.body[rk + e];
  }
  const float u = a.u[jl];
#pragma unroll
  for (int e = 0; e < 9; ++e) old[e] = (on && a.add) ? a.g[row + e] : 0.f;
  const bool head = l == 0 && f < a.F;
  const float old_share = (head && a.add) ? a.g[(size_t)a.F * 207 + f] : 0.f;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (a.norm_body) {
      gs6d_forward(raw[k], R[k]);
    } else {
#pragma unroll
      for (int e = 0; e < 9; ++e) R[k][e] = raw[k][e];
    }
  }
  const bool v0 = f <= a.F - 3, v1 = f >= 1 && f <= a.F - 2, v2 = f >= 2;  // a_s, a_{s-1}, a_{s-2} exist
  const bool zero = u == 0.f;
  const float wc = a.cg * u;
  float dR[9], sq = 0.f;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const float a0 = v0 ? (R[2][e] - 2.f * R[3][e]) + R[4][e] : 0.f;
    const float a1 = v1 ? (R[1][e] - 2.f * R[2][e]) + R[3][e] : 0.f;
    const float a2 = v2 ? (R[0][e] - 2.f * R[1][e]) + R[2][e] : 0.f;
    dR[e] = wc * ((a0 - 2.f * a1) + a2);
    sq = fmaf(a0, a0, sq);
  }
  float out[9];
  if (a.norm_body) {
    float da[6];
    gs6d_backward(raw[2], dR, da);
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = zero ? old[e] : old[e] + da[e];
    out[6] = old[6]; out[7] = old[7]; out[8] = old[8];
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) out[e] = zero ? old[e] : old[e] + dR[e];
  }
  if (on) {
#pragma unroll
    for (int e = 0; e < 9; ++e) a.g[row + e] = out[e];
  }
  // the frame's share: the lanes' weighted sums through a fixed butterfly inside the 32-lane half
  float part = (on && v0 && !zero) ? u * sq : 0.f;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  if (head) a.g[(size_t)a.F * 207 + f] = old_share + a.cl * part;
}

// ----------------------------------------------------------------------------------------------------
// EXTENSION (not reference behaviour; uuo_fit_set_keypoints2d): a 2D key-point reprojection term on the 24 kinematic joints
// J[t][j] = G_j^t + trans_t.  Frame t carries a pinhole camera in world axes, cam[t] = (A 3x3 row-major, b, fx, fy, cx, cy),
// targets y[t][j] and confidences c[t][j] >= 0:
//   p = A J + b,  u = (fx p_x / p_z + cx, fy p_y / p_z + cy),  r = u - y,  s = |r|^2,
//   valid = c > 0 and p finite and p_z >= min_depth,
//   loss += w / (48 F) sum_valid c rho(s)       (rho(s) = s q, q = sigma^2 / (sigma^2 + s); sigma = 0: rho(s) = s)
//   k = 2 w c rho'(s) / (48 F)                  (rho' = q^2; sigma = 0: 1)
//   dL/dp = k (r_x fx / p_z, r_y fy / p_z, -(r_x fx p_x + r_y fy p_y) / p_z^2),  dL/dJ = A^T dL/dp.
// An invalid pair contributes exact zeros (selected, not multiplied).
// k_keypoint2d_fwd delivers dL/dG_j^t and the frames' shares through the buffer of the self-penetration term, [F][24][3] and
// [F] behind them, which the temporal instantiations add to uj -- from where the translation takes the joints' sum -- and to
// slot 3 (cap_up != null): no existing kernel changes.  add == 0: it writes the buffer; add != 0 (the capsules are on,
// k_capsule_fwd of this evaluation ran before it on the same stream): it adds to it.
// The shape of k_limit_fwd: 32 lanes per frame, two frames per 64-thread block.  Lane l < 24 of a half takes joint l: its G^t
// of the frame's FrameLds (as the closure's forward or k_pose_prep left them), the frame's translation and camera row (the
// lanes of a half read the same 19 floats), its target and confidence (and with add its three old gradients; lane 0 the old
// share) in one round trip.  The frame's share: every lane forms c rho(s), then a fixed xor butterfly (16, 8, .. 1) inside the
// half adds the lanes (lanes 24 .. 31 and invalid pairs hold zeros).  No atomics, no LDS: bit-reproducible.
// ----------------------------------------------------------------------------------------------------
struct Keypoint2dArgs {
  uuo_gptr<const float> frames;   // [F][FrameLds]
  uuo_gptr<const float> trans;    // [F][3] or null
  uuo_gptr<const float> cam;      // [F][16]
  uuo_gptr<const float> targets;  // [F][24][2]
  uuo_gptr<const float> conf;     // [F][24]
  int F, add;
  float cl, cg;                   // w / (48 F), 2 w / (48 F)
  float rs2, min_depth;           // sigma^2 (0 = the square)
  uuo_gptr<float> up;             // [F][24][3] gradients, then [F] shares: written (add == 0) or added to
};
__global__ __launch_bounds__(64) void k_keypoint2d_fwd(Keypoint2dArgs a) {
  constexpr int NW = sizeof(FrameLds) / 4, GT = offsetof(FrameLds, Gt) / 4;
  const int half = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int f = blockIdx.x * UUO_LIM_FPB + half;
  const bool on = f < a.F && l < UUO_NUM_JOINTS;
  const size_t fr = on ? (size_t)f : 0, row = on ? (size_t)f * UUO_NUM_JOINTS + l : 0;
  const float* gt = a.frames + fr * NW + GT + (on ? l * 3 : 0);
  const float gx = gt[0], gy = gt[1], gz = gt[2];
  const float tx = a.trans ? a.trans[fr * 3] : 0.f, ty = a.trans ? a.trans[fr * 3 + 1] : 0.f, tz = a.trans ? a.trans[fr * 3 + 2] : 0.f;
  const float* cm = a.cam + fr * 16;
  const float A0 = cm[0], A1 = cm[1], A2 = cm[2], A3 = cm[3], A4 = cm[4], A5 = cm[5], A6 = cm[6], A7 = cm[7], A8 = cm[8];
  const float b0 = cm[9], b1 = cm[10], b2 = cm[11], fx = cm[12], fy = cm[13], cx = cm[14], cy = cm[15];
  const float y0 = a.targets[row * 2], y1 = a.targets[row * 2 + 1];
  const float c = on ? a.conf[row] : 0.f;
  const bool head = l == 0 && f < a.F;
  const float old0 = (on && a.add) ? a.up[row * 3] : 0.f, old1 = (on && a.add) ? a.up[row * 3 + 1] : 0.f,
              old2 = (on && a.add) ? a.up[row * 3 + 2] : 0.f;
  const float old_share = (head && a.add) ? a.up[(size_t)a.F * 72 + f] : 0.f;
  const float jx = gx + tx, jy = gy + ty, jz = gz + tz;
  const float px = fmaf(A2, jz, fmaf(A1, jy, A0 * jx)) + b0;
  const float py = fmaf(A5, jz, fmaf(A4, jy, A3 * jx)) + b1;
  const float pz = fmaf(A8, jz, fmaf(A7, jy, A6 * jx)) + b2;
  // (false for NaN; the setters' bound: a magnitude in (3.0e38, FLT_MAX] counts as not finite here, where torch.isfinite of the
  // composed term lets it pass -- no camera puts a joint there)
  const bool finite = fabsf(px) <= 3.0e38f && fabsf(py) <= 3.0e38f && fabsf(pz) <= 3.0e38f;
  const bool valid = c > 0.f && finite && pz >= a.min_depth;
  const float iz = 1.f / (valid ? pz : 1.f);  // (keeps the quotients of the unused branch finite)
  const float rx = fmaf(fx * px, iz, cx) - y0, ry = fmaf(fy * py, iz, cy) - y1;
  const float s = rx * rx + ry * ry;
  const float q = (a.rs2 > 0.f) ? a.rs2 / (a.rs2 + s) : 1.f;
  const float k = (a.cg * c) * (q * q);
  const float ax = rx * fx, ay = ry * fy;
  const float dx = k * (ax * iz), dy = k * (ay * iz), dz = -(k * ((ax * px + ay * py) * (iz * iz)));
  const float g0 = valid ? fmaf(A6, dz, fmaf(A3, dy, A0 * dx)) : 0.f;
  const float g1 = valid ? fmaf(A7, dz, fmaf(A4, dy, A1 * dx)) : 0.f;
  const float g2 = valid ? fmaf(A8, dz, fmaf(A5, dy, A2 * dx)) : 0.f;
  if (on) {
    a.up[row * 3] = old0 + g0;
    a.up[row * 3 + 1] = old1 + g1;
    a.up[row * 3 + 2] = old2 + g2;
  }
  // the frame's share: the lanes' c rho(s) through a fixed butterfly inside the 32-lane half
  float part = valid ? c * (s * q) : 0.f;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
  if (head) a.up[(size_t)a.F * 72 + f] = old_share + a.cl * part;
}

// The side terms that are on, in this order on stream s, once the frames' FrameLds of this evaluation are there.  cap_up and
// lim_g are shared: the first kernel of an evaluation to reach a buffer writes it, the later ones add to it.
void uuo_launch_side_terms(uuo_fit* fit, hipStream_t s, int F, const UuoPoseSrc& src, const float* d_pose, const float* d_o_pose,
                           float w_pose, UuoSideTerms on) {
  const uuo_model* m = fit->model;
  bool cap_up_written = false, lim_g_written = false;  // in this evaluation
  if (on.floor) {
    FloorFwdArgs b;
    std::memset(&b, 0, sizeof(b));
    b.PT = m->PT; b.ST = m->ST; b.vt = m->vt; b.Ww = m->Ww; b.Wi = m->Wi;
    b.V = m->V; b.F = F; b.K = fit->floor_k; b.KL = fit->floor_kl;
    b.frames = fit->frames;
    b.trans = src.trans;
    b.vids = fit->floor_vids;
    b.contacts = fit->floor_contacts;
    b.h = fit->floor_height;
    b.cpen = (float)((double)fit->floor_pen / ((double)F * (double)fit->floor_k));
    b.ccon = (float)((double)fit->floor_con / (2.0 * (double)F));
    b.up = fit->floor_up;
    b.loss = uuo_floor_up_shares(fit);
    hipLaunchKernelGGL(k_floor_fwd, dim3(F), dim3(64), 0, s, b);
  }
  if (on.caps) {
    CapsFwdArgs b;
    std::memset(&b, 0, sizeof(b));
    b.frames = fit->frames;
    b.tab = static_cast<const int32_t*>(fit->cap_tab.dev);
    b.geom = reinterpret_cast<const float*>(static_cast<const int32_t*>(fit->cap_tab.dev) + UUO_CAPS_TAB_INTS);
    b.C = fit->cap_c; b.P = fit->cap_p;
    b.cl = (float)((double)fit->cap_w / (double)F);
    b.cg = (float)(2.0 * (double)fit->cap_w / (double)F);
    b.up = fit->cap_up;
    b.loss = uuo_cap_up_shares(fit);
    hipLaunchKernelGGL(k_capsule_fwd, dim3(F), dim3(64), 0, s, b);
    fit->cap_tab.note_reader(s);
    cap_up_written = true;
  }
  if (on.kp) {
    Keypoint2dArgs b;
    std::memset(&b, 0, sizeof(b));
    b.frames = fit->frames;
    b.trans = src.trans;
    b.cam = fit->kp_cam;
    b.targets = fit->kp_targets;
    b.conf = fit->kp_conf;
    b.F = F;
    b.add = cap_up_written ? 1 : 0;
    b.cl = (float)((double)fit->kp_w / (48.0 * (double)F));
    b.cg = (float)(2.0 * (double)fit->kp_w / (48.0 * (double)F));
    b.rs2 = (float)((double)fit->kp_sigma * (double)fit->kp_sigma);
    b.min_depth = fit->kp_min_depth;
    b.up = fit->cap_up;
    hipLaunchKernelGGL(k_keypoint2d_fwd, dim3((F + UUO_LIM_FPB - 1) / UUO_LIM_FPB), dim3(64), 0, s, b);
    cap_up_written = true;
  }
  if (on.limits) {
    LimitFwdArgs b;
    std::memset(&b, 0, sizeof(b));
    b.body = src.body;
    b.tab = static_cast<const float*>(fit->lim_tab.dev);
    b.F = F;
    b.norm_body = src.norm_body;
    b.cl = (float)((double)fit->lim_w / (double)F);
    b.cg = (float)(2.0 * (double)fit->lim_w / (double)F);
    b.g = fit->lim_g;
    b.loss = uuo_lim_g_shares(fit);
    hipLaunchKernelGGL(k_limit_fwd, dim3((F + UUO_LIM_FPB - 1) / UUO_LIM_FPB), dim3(64), 0, s, b);
    fit->lim_tab.note_reader(s);
    lim_g_written = true;
  }
  if (on.pose_gmm) {
    PoseGmmArgs b;
    std::memset(&b, 0, sizeof(b));
    b.body = src.body;
    b.tab = static_cast<const float*>(fit->gmm_tab.dev);
    b.F = F;
    b.K = fit->gmm_k;
    b.norm_body = src.norm_body;
    b.add = lim_g_written ? 1 : 0;
    b.cw = (float)((double)fit->gmm_w / (double)F);
    b.g = fit->lim_g;
    b.win = fit->gmm_win;
    hipLaunchKernelGGL(k_pose_gmm, dim3((F + UUO_GMM_FPB - 1) / UUO_GMM_FPB), dim3(64 * UUO_GMM_WAVES), 0, s, b);
    fit->gmm_tab.note_reader(s);
    lim_g_written = true;
  }
  if (on.pose_accel) {  // (the caller has seen F >= 3)
    PoseAccelArgs b;
    std::memset(&b, 0, sizeof(b));
    b.body = src.body;
    b.u = static_cast<const float*>(fit->pacc_tab.dev);
    b.F = F;
    b.norm_body = src.norm_body;
    b.add = lim_g_written ? 1 : 0;
    b.cl = (float)((double)fit->pacc_w / ((double)(F - 2) * 207.0));
    b.cg = (float)(2.0 * (double)fit->pacc_w / ((double)(F - 2) * 207.0));
    b.g = fit->lim_g;
    hipLaunchKernelGGL(k_pose_accel, dim3((F + UUO_LIM_FPB - 1) / UUO_LIM_FPB), dim3(64), 0, s, b);
    fit->pacc_tab.note_reader(s);
    lim_g_written = true;
  }
  if (on.prior) {
    PriorConfArgs b;
    std::memset(&b, 0, sizeof(b));
    b.body = d_pose;
    b.target = d_o_pose;
    b.w = fit->prior_w;
    b.F = F;
    b.add = lim_g_written ? 1 : 0;
    b.cl = (float)((double)w_pose / ((double)F * 207.0));
    b.cg = (float)(2.0 * (double)w_pose / ((double)F * 207.0));
    b.g = fit->lim_g;
    hipLaunchKernelGGL(k_prior_conf, dim3((F + UUO_LIM_FPB - 1) / UUO_LIM_FPB), dim3(64), 0, s, b);
  }
}

// the two shared accumulation buffers, allocated by the first setter that needs one: [F][207] (lim_g) or [F][72] (cap_up)
// gradients, then the [F] loss shares (uuo_lim_g_shares, uuo_cap_up_shares)
static int ensure_lim_g(uuo_fit* fit) {
  if (!fit->lim_g) UUO_HIP_CHECK(hipMalloc((void**)&fit->lim_g, ((size_t)fit->F * 207 + fit->F) * sizeof(float)));
  return 0;
}
static int ensure_cap_up(uuo_fit* fit) {
  if (!fit->cap_up) UUO_HIP_CHECK(hipMalloc((void**)&fit->cap_up, ((size_t)fit->F * 72 + fit->F) * sizeof(float)));
  return 0;
}

extern "C" int uuo_fit_set_joint_accel(uuo_fit_t* fit, float w) {
  UUO_REQUIRE(fit, "uuo_fit_set_joint_accel: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_joint_accel: the weight must be 0 (off) or a positive finite number");
  UUO_REQUIRE(w == 0.f || !uuo_recorder, "uuo_fit_set_joint_accel: lock-step batches do not carry the joint-acceleration term");
  fit->joint_accel = w;
  return 0;
}

extern "C" int uuo_fit_set_foot_lock(uuo_fit_t* fit, float w, const float* d_contacts) {
  UUO_REQUIRE(fit, "uuo_fit_set_foot_lock: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_foot_lock: the weight must be 0 (off) or a positive finite number");
  UUO_REQUIRE(w == 0.f || d_contacts, "uuo_fit_set_foot_lock: a positive weight needs the contact labels [F][2] on the device");
  UUO_REQUIRE(w == 0.f || !uuo_recorder, "uuo_fit_set_foot_lock: lock-step batches do not carry the foot-lock term");
  fit->foot_lock = w;
  fit->foot_contacts = (w == 0.f) ? nullptr : d_contacts;
  return 0;
}

extern "C" int uuo_fit_set_floor(uuo_fit_t* fit, float w_pen, float w_con, float height, const int32_t* d_vids, int32_t k_left,
                                 int32_t k_right, const float* d_contacts) {
  UUO_REQUIRE(fit, "uuo_fit_set_floor: null fit");
  UUO_REQUIRE((w_pen == 0.f || (w_pen > 0.f && w_pen <= 3.0e38f)) && (w_con == 0.f || (w_con > 0.f && w_con <= 3.0e38f)),
              "uuo_fit_set_floor: the weights must be 0 (off) or positive finite numbers");
  if (w_pen == 0.f && w_con == 0.f) {  // off: nothing else is looked at
    fit->floor_pen = fit->floor_con = fit->floor_height = 0.f;
    fit->floor_k = fit->floor_kl = 0;
    fit->floor_vids = nullptr;
    fit->floor_contacts = nullptr;
    return 0;
  }
  UUO_REQUIRE(height >= -3.0e38f && height <= 3.0e38f, "uuo_fit_set_floor: the plane height must be a finite number of metres");
  UUO_REQUIRE(k_left >= 1 && k_right >= 1, "uuo_fit_set_floor: every foot needs at least one sole point");
  UUO_REQUIRE(k_left + (long long)k_right >= 2 && k_left + (long long)k_right <= UUO_FLOOR_MAXK,
              "uuo_fit_set_floor: 2 .. 16 sole points (k_left + k_right)");
  UUO_REQUIRE(d_vids, "uuo_fit_set_floor: the sole points' vertex ids [k_left + k_right] on the device are required");
  UUO_REQUIRE(w_con == 0.f || d_contacts, "uuo_fit_set_floor: a positive contact weight needs the contact labels [F][2] on the device");
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_floor: lock-step batches do not carry the floor-contact term");
  const int K = k_left + k_right;
  int32_t h_vids[UUO_FLOOR_MAXK];
  UUO_HIP_CHECK(hipMemcpy(h_vids, d_vids, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int k = 0; k < K; ++k)
    UUO_REQUIRE(h_vids[k] >= 0 && h_vids[k] < fit->model->V, "uuo_fit_set_floor: a sole point's vertex id is outside [0, V)");
  if (!fit->floor_up)  // [F][16][3] upstream gradients + [F] loss shares (k_floor_fwd -> the backward); first use
    UUO_HIP_CHECK(hipMalloc((void**)&fit->floor_up, ((size_t)fit->F * UUO_FLOOR_MAXK * 3 + fit->F) * sizeof(float)));
  fit->floor_pen = w_pen;
  fit->floor_con = w_con;
  fit->floor_height = height;
  fit->floor_k = K;
  fit->floor_kl = k_left;
  fit->floor_vids = d_vids;
  fit->floor_contacts = (w_con == 0.f) ? nullptr : d_contacts;
  return 0;
}

extern "C" int uuo_fit_set_capsules(uuo_fit_t* fit, float w, int32_t n_caps, const int32_t* h_cap_joints, const float* h_cap_geom,
                                    int32_t n_pairs, const int32_t* h_pairs) {
  UUO_REQUIRE(fit, "uuo_fit_set_capsules: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_capsules: the weight must be 0 (off) or a positive finite number");
  if (w == 0.f) {  // off: nothing else is looked at (the tables stay for the next call with the same lists)
    fit->cap_w = 0.f;
    return 0;
  }
  UUO_REQUIRE(n_caps >= 1 && n_caps <= UUO_CAPS_MAXC, "uuo_fit_set_capsules: 1 .. 32 capsules");
  UUO_REQUIRE(n_pairs >= 1 && n_pairs <= UUO_CAPS_MAXP, "uuo_fit_set_capsules: 1 .. 256 pairs");
  UUO_REQUIRE(h_cap_joints && h_cap_geom && h_pairs,
              "uuo_fit_set_capsules: a positive weight needs the capsules' joints [C][2], geometry [C][3] and the pairs [P][2] (host arrays)");
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_capsules: lock-step batches do not carry the self-penetration term");
  const int C = n_caps, P = n_pairs;
  for (int c = 0; c < C; ++c) {
    const int u = h_cap_joints[c * 2], v = h_cap_joints[c * 2 + 1];
    UUO_REQUIRE(u >= 0 && u < UUO_NUM_JOINTS && v >= 0 && v < UUO_NUM_JOINTS, "uuo_fit_set_capsules: a capsule's joint id is outside [0, 24)");
    UUO_REQUIRE(u != v, "uuo_fit_set_capsules: a capsule needs two different joints");
    const float al = h_cap_geom[c * 3], be = h_cap_geom[c * 3 + 1], r = h_cap_geom[c * 3 + 2];
    UUO_REQUIRE(al >= -3.0e38f && al <= 3.0e38f && be >= -3.0e38f && be <= 3.0e38f,
                "uuo_fit_set_capsules: a capsule's alpha and beta must be finite");
    UUO_REQUIRE(r > 0.f && r <= 3.0e38f, "uuo_fit_set_capsules: a capsule's radius must be a positive finite number of metres");
  }
  for (int k = 0; k < P; ++k) {
    const int i = h_pairs[k * 2], j = h_pairs[k * 2 + 1];
    UUO_REQUIRE(i >= 0 && i < C && j >= 0 && j < C, "uuo_fit_set_capsules: a pair's capsule index is outside [0, C)");
    UUO_REQUIRE(i != j, "uuo_fit_set_capsules: a pair needs two different capsules");
  }
  if (const int rc = ensure_cap_up(fit)) return rc;
  // what the table is built from: the caller's lists (zero-padded, so that equal structs are equal lists)
  struct {
    int32_t C, P, joints[UUO_CAPS_MAXC * 2], pairs[UUO_CAPS_MAXP * 2];
    float geom[UUO_CAPS_MAXC * 3];
  } key;
  std::memset(&key, 0, sizeof(key));
  key.C = C;
  key.P = P;
  std::memcpy(key.joints, h_cap_joints, (size_t)C * 2 * sizeof(int32_t));
  std::memcpy(key.pairs, h_pairs, (size_t)P * 2 * sizeof(int32_t));
  std::memcpy(key.geom, h_cap_geom, (size_t)C * 3 * sizeof(float));
  struct Image {  // (the kernel fetches the whole table)
    int32_t tab[UUO_CAPS_TAB_INTS];
    float geom[UUO_CAPS_MAXC * 3];
  };
  const int rc = fit->cap_tab.replace_if_changed(&fit->upload_stream, &fit->cap_w, &key, sizeof(key), sizeof(Image), [&]() -> const void* {
    // the joint -> (pair, end) table, CSR: joint jj's rows list 4 k + end in pair order, inside a pair in the order
    // u_i (end 0), v_i (1), u_j (2), v_j (3) -- the order in which k_capsule_fwd sums
    static thread_local Image im;
    std::memset(&im, 0, sizeof(im));
    std::memcpy(im.tab, key.joints, sizeof(key.joints));
    std::memcpy(im.tab + UUO_CAPS_TAB_PAIRS, key.pairs, sizeof(key.pairs));
    std::memcpy(im.geom, key.geom, sizeof(key.geom));
    int n = 0;
    for (int jj = 0; jj < UUO_NUM_JOINTS; ++jj) {
      im.tab[UUO_CAPS_TAB_OFF + jj] = n;
      for (int k = 0; k < P; ++k)
        for (int end = 0; end < 4; ++end)
          if (h_cap_joints[h_pairs[k * 2 + (end >> 1)] * 2 + (end & 1)] == jj) im.tab[UUO_CAPS_TAB_ENT + n++] = 4 * k + end;
    }
    im.tab[UUO_CAPS_TAB_OFF + UUO_NUM_JOINTS] = n;  // = 4 P
    return &im;
  });
  if (rc) return rc;
  fit->cap_c = C;
  fit->cap_p = P;
  fit->cap_w = w;
  return 0;
}

extern "C" int uuo_fit_set_keypoints2d(uuo_fit_t* fit, float w, float sigma, float min_depth, const float* d_cam,
                                       const float* d_targets, const float* d_conf) {
  UUO_REQUIRE(fit, "uuo_fit_set_keypoints2d: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_keypoints2d: the weight must be 0 (off) or a positive finite number");
  if (w == 0.f) {  // off: nothing else is looked at
    fit->kp_w = fit->kp_sigma = fit->kp_min_depth = 0.f;
    fit->kp_cam = fit->kp_targets = fit->kp_conf = nullptr;
    return 0;
  }
  // (sigma > 0: sigma^2 has to be a normal fp32 value, as uuo_problem_t.robust_sigma's)
  UUO_REQUIRE(sigma == 0.f || (sigma >= 1.0e-18f && sigma <= 1.0e18f),
              "uuo_fit_set_keypoints2d: sigma must be 0 (the square) or a positive finite number in [1e-18, 1e18]");
  UUO_REQUIRE(min_depth > 0.f && min_depth <= 3.0e38f, "uuo_fit_set_keypoints2d: min_depth must be a positive finite number");
  UUO_REQUIRE(d_cam && d_targets && d_conf,
              "uuo_fit_set_keypoints2d: a positive weight needs the cameras [F][16], the targets [F][24][2] and the confidences "
              "[F][24] on the device");
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_keypoints2d: lock-step batches do not carry the key-point reprojection term");
  if (const int rc = ensure_cap_up(fit)) return rc;  // (the buffer k_keypoint2d_fwd fills is the self-penetration term's)
  fit->kp_w = w;
  fit->kp_sigma = sigma;
  fit->kp_min_depth = min_depth;
  fit->kp_cam = d_cam;
  fit->kp_targets = d_targets;
  fit->kp_conf = d_conf;
  return 0;
}

extern "C" int uuo_fit_set_joint_limits(uuo_fit_t* fit, float w, const float* h_lo, const float* h_hi) {
  UUO_REQUIRE(fit, "uuo_fit_set_joint_limits: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_joint_limits: the weight must be 0 (off) or a positive finite number");
  if (w == 0.f) {  // off: nothing else is looked at (the table stays for the next call with the same bounds)
    fit->lim_w = 0.f;
    return 0;
  }
  UUO_REQUIRE(h_lo && h_hi, "uuo_fit_set_joint_limits: a positive weight needs the bounds lo [23][3] and hi [23][3] (host arrays)");
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_joint_limits: lock-step batches do not carry the joint-angle limit term");
  for (int i = 0; i < 69; ++i) {
    const float lo = h_lo[i], hi = h_hi[i];
    UUO_REQUIRE(lo == lo && hi == hi, "uuo_fit_set_joint_limits: a bound is NaN");
    UUO_REQUIRE(lo <= 3.0e38f, "uuo_fit_set_joint_limits: a lower bound of +inf admits no angle (-inf = no bound)");
    UUO_REQUIRE(hi >= -3.0e38f, "uuo_fit_set_joint_limits: an upper bound of -inf admits no angle (+inf = no bound)");
    UUO_REQUIRE(lo <= hi, "uuo_fit_set_joint_limits: lo > hi");
  }
  if (const int rc = ensure_lim_g(fit)) return rc;
  static thread_local float h_tab[2 * 69];
  std::memcpy(h_tab, h_lo, 69 * sizeof(float));
  std::memcpy(h_tab + 69, h_hi, 69 * sizeof(float));
  if (const int rc = fit->lim_tab.replace_if_changed(&fit->upload_stream, &fit->lim_w, h_tab, sizeof(h_tab))) return rc;
  fit->lim_w = w;
  return 0;
}

extern "C" int uuo_fit_set_pose_gmm(uuo_fit_t* fit, float w, int K, const float* h_means, const float* h_chol, const float* h_offsets) {
  UUO_REQUIRE(fit, "uuo_fit_set_pose_gmm: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_pose_gmm: the weight must be 0 (off) or a positive finite number");
  if (w == 0.f) {  // off: nothing else is looked at (the table stays for the next call with the same mixture)
    fit->gmm_w = 0.f;
    return 0;
  }
  UUO_REQUIRE(K >= 1 && K <= UUO_GMM_MAXK, "uuo_fit_set_pose_gmm: 1 .. 16 components");
  UUO_REQUIRE(h_means && h_chol && h_offsets,
              "uuo_fit_set_pose_gmm: a positive weight needs the means [K][69], the factors A_k [K][69][69] and the offsets [K] (host arrays)");
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_pose_gmm: lock-step batches do not carry the pose mixture term");
  const auto finite = [](float v) { return v >= -3.0e38f && v <= 3.0e38f; };  // (false for NaN)
  for (int i = 0; i < K * 69; ++i) UUO_REQUIRE(finite(h_means[i]), "uuo_fit_set_pose_gmm: a mean is NaN or not finite");
  for (int i = 0; i < K * 69 * 69; ++i) UUO_REQUIRE(finite(h_chol[i]), "uuo_fit_set_pose_gmm: an entry of a factor A_k is NaN or not finite");
  for (int i = 0; i < K; ++i) UUO_REQUIRE(finite(h_offsets[i]), "uuo_fit_set_pose_gmm: an offset is NaN or not finite");
  for (int k = 0; k < K; ++k)
    for (int r = 0; r < 69; ++r)
      UUO_REQUIRE(h_chol[((size_t)k * 69 + r) * 69 + r] > 0.f, "uuo_fit_set_pose_gmm: a diagonal entry of a factor A_k is not positive");
  for (int i = 0; i < K; ++i) UUO_REQUIRE(h_offsets[i] >= 0.f, "uuo_fit_set_pose_gmm: an offset is negative (they are shifted so that the least is 0)");
  if (const int rc = ensure_lim_g(fit)) return rc;  // (the buffer k_pose_gmm fills is the joint-angle limit term's)
  // the winners, F ints and one store a frame: only the checkers read them (uuo_debug_pose_gmm_state), but the tests evaluate
  // through the product flavour and hand its workspace to the debug flavour's hook, so the product keeps the buffer too
  if (!fit->gmm_win) UUO_HIP_CHECK(hipMalloc((void**)&fit->gmm_win, (size_t)fit->F * sizeof(int32_t)));
  // what the table is built from: K and the caller's arrays.  _arm() makes this call before every evaluation and solve with the
  // arrays of the call before, so that case compares them with the mirror where they lie (three memcmp, 155 KB at K = 8: about
  // 10 us of host time) and copies nothing
  const size_t n_mu = (size_t)K * 69, n_a = (size_t)K * 69 * 69;
  if (fit->gmm_tab.valid && fit->gmm_tab.mirror.size() == (1 + n_mu + n_a + K) * sizeof(float)) {
    const float* mir = reinterpret_cast<const float*>(fit->gmm_tab.mirror.data());
    if (mir[0] == (float)K && std::memcmp(mir + 1, h_means, n_mu * sizeof(float)) == 0 &&
        std::memcmp(mir + 1 + n_mu, h_chol, n_a * sizeof(float)) == 0 &&
        std::memcmp(mir + 1 + n_mu + n_a, h_offsets, (size_t)K * sizeof(float)) == 0) {
      fit->gmm_k = K;
      fit->gmm_w = w;
      return 0;
    }
  }
  static thread_local std::vector<float> key, image;
  key.resize(1 + (size_t)K * (69 + 69 * 69 + 1));
  key[0] = (float)K;
  std::memcpy(key.data() + 1, h_means, (size_t)K * 69 * sizeof(float));
  std::memcpy(key.data() + 1 + (size_t)K * 69, h_chol, (size_t)K * 69 * 69 * sizeof(float));
  std::memcpy(key.data() + 1 + (size_t)K * (69 + 69 * 69), h_offsets, (size_t)K * sizeof(float));
  const int rc = fit->gmm_tab.replace_if_changed(&fit->upload_stream, &fit->gmm_w, key.data(), key.size() * sizeof(float),
                                                 (size_t)UUO_GMM_TAB_FLOATS * sizeof(float), [&]() -> const void* {
    // the lower triangles row-major ((r, c) at r (r + 1) / 2 + c: what is above the diagonal is not read), every array at its
    // K = 16 place, zeros behind
    image.assign(UUO_GMM_TAB_FLOATS, 0.f);
    for (int k = 0; k < K; ++k) {
      for (int r = 0; r < 69; ++r)
        for (int c = 0; c <= r; ++c) image[(size_t)k * UUO_GMM_TRI + r * (r + 1) / 2 + c] = h_chol[((size_t)k * 69 + r) * 69 + c];
      std::memcpy(image.data() + UUO_GMM_TAB_MEANS + k * 69, h_means + k * 69, 69 * sizeof(float));
      image[UUO_GMM_TAB_OFFS + k] = h_offsets[k];
    }
    return image.data();
  });
  if (rc) return rc;
  fit->gmm_k = K;
  fit->gmm_w = w;
  return 0;
}

extern "C" int uuo_fit_set_pose_accel(uuo_fit_t* fit, float w, const float* h_joint_weights) {
  UUO_REQUIRE(fit, "uuo_fit_set_pose_accel: null fit");
  UUO_REQUIRE(w == 0.f || (w > 0.f && w <= 3.0e38f), "uuo_fit_set_pose_accel: the weight must be 0 (off) or a positive finite number");
  if (w == 0.f) {  // off: nothing else is looked at (the table stays for the next call with the same weights)
    fit->pacc_w = 0.f;
    return 0;
  }
  UUO_REQUIRE(!uuo_recorder, "uuo_fit_set_pose_accel: lock-step batches do not carry the pose-acceleration term");
  static thread_local float h_tab[23];
  for (int i = 0; i < 23; ++i) {
    const float v = h_joint_weights ? h_joint_weights[i] : 1.f;  // (null = ones)
    UUO_REQUIRE(v >= 0.f && v <= 3.0e38f, "uuo_fit_set_pose_accel: a joint weight is NaN, negative or not finite");
    h_tab[i] = v;
  }
  if (const int rc = ensure_lim_g(fit)) return rc;  // (the buffer k_pose_accel fills is the joint-angle limit term's)
  if (const int rc = fit->pacc_tab.replace_if_changed(&fit->upload_stream, &fit->pacc_w, h_tab, sizeof(h_tab))) return rc;
  fit->pacc_w = w;
  return 0;
}

extern "C" int uuo_fit_set_prior_weights(uuo_fit_t* fit, const float* d_weights) {
  UUO_REQUIRE(fit, "uuo_fit_set_prior_weights: null fit");
  UUO_REQUIRE(!d_weights || !uuo_recorder, "uuo_fit_set_prior_weights: lock-step batches do not carry the pose prior's weights");
  if (d_weights)  // (the buffer k_prior_conf fills is the joint-angle limit term's)
    if (const int rc = ensure_lim_g(fit)) return rc;
  fit->prior_w = d_weights;
  return 0;
}
