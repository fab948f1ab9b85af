// Unsupervised training loss for gfx950: brightness constancy over the non-occluded pixels plus an edge-aware smoothness prior on the flow,
// both directions in ONE launch per direction of differentiation, the per-sample rows and the loss in fp64 from a one-workgroup finalise.
//
// Composed from flow_warp and eager tensor operations this is dozens of launches per scale and direction, each with a temporary of the
// full map.  Here a thread streams its own pixels (flow, occ, the C channels of its own image), gathers the four taps per channel of the
// other image at each target, evaluates the smoothness terms its pixels own from the neighbours' flows and keeps its sums in registers;
// then, as in flow_consistency.hip: wave64 reduction -> LDS -> one fp64 partial row per workgroup, and a finalise that adds a sample's
// partial rows in index order, the sample rows in sample order, and forms the loss.  The backward is a gather of the same shape without
// the reduction: a pixel's data gradient depends on that pixel alone, its smoothness gradient on the terms owned by itself and by its
// neighbours one step away along each axis, which the thread evaluates again.  No atomics on floats, nothing read back by the host.
//
// A work item is (direction, sample, chunk), B chunks per sample, B from H * W alone: a sample's row has the same bits alone and in any
// batch.  A thread owns one pixel per step, or four neighbouring pixels of a row where W is a multiple of 4.  On the four-pixel path the
// whole neighbourhood of the unit -- row y over x - 4 .. x + 7 and the rows y - 2 .. y + 2 over x .. x + 3, of both flow planes and, with
// an edge weight, of every channel of the own image -- is loaded as four-pixel accesses (16-byte ones where every pointer given is
// 16-byte aligned, four 4-byte ones otherwise: the same values in the same order) and every term is evaluated once per thread; on the
// one-pixel path every term loads what it reads.  Either way the neighbour rows come from L2, not from LDS: the workgroups of a sample
// walk adjoining 1024-pixel slabs at the same time, so a neighbour row is a line another workgroup has just streamed, and HBM sees each
// byte once (DESIGN.md section 3.17 has the byte count).  Every operation is rounded on its own (fp contract off):
// include/flownet2_hip_unsup_loss.h states the arithmetic, and both paths carry it out term by term, so their bits are the same.
//
// Reads stay inside the sample: a row or a four-pixel group of the neighbourhood is loaded only where it lies inside the plane, a
// smoothness term is formed only where its pixels are, and the tap indices are formed only after the finite, occlusion and inside tests,
// from a coordinate in [0, W) x [0, H), and clamped to W - 1 and H - 1.
#include "stream_reduce.hpp"
#include "../../include/flownet2_hip_unsup_loss.h"

#pragma clang fp contract(off)

namespace fn2 {

using namespace stream;

constexpr int kUlK = FN2_UNSUP_LOSS_K;                 // every column is a sum
constexpr int kUlMaxC = 4;
enum { kUlCounted = 0, kUlOccluded, kUlOutside, kUlNonfinite };

struct UlArgs {
  const float* img[2];         // direction d: Ia = img[d], Io = img[1 - d]
  const float* flow[2];
  const float* occ[2];
  float* diff[2];              // backward
  double* partial;             // forward: [dirs][N][B][K]
  double* results;             // forward: [2][N + 1][K]
  const double* totals;        // backward: the forward's results
  float* loss;
  const float* total_diff;
  int N, C, H, W;
  int chunks;                  // B
  int dirs;                    // directions run: 1 or 2
  int quad;                    // W % 4 == 0: four pixels per thread and step
  int vec;                     // and every pointer given 16-byte aligned: 16-byte loads / stores
  int order;
  float dw, sw, eps_d, gam_d, eps_s, gam_s, edge, mult;
};

// one (direction, sample): the own flow's planes, the own and the other image (C planes each), the occ plane or NULL
struct UlSample {
  const float* __restrict__ u;
  const float* __restrict__ v;
  const float* __restrict__ Ia;
  const float* __restrict__ Io;
  const float* __restrict__ occ;
};

__device__ __forceinline__ float ul_psi(float t, float eps, float gam) {
  const float r = t * t + eps * eps;
  return gam == 0.5f ? sqrtf(r) : powf(r, gam);
}

__device__ __forceinline__ float ul_dpsi(float t, float eps, float gam) {
  const float r = t * t + eps * eps;
  return gam == 0.5f ? t / sqrtf(r) : ((2.0f * gam) * t) * powf(r, gam - 1.0f);
}

struct UlData {
  int cls;
  float e, su, sv;             // the data term; with GRAD the sums Su, Sv of the header
};

// The data term of pixel (x, y): fu, fv its own raw flow, oc its occ value (0 without a plane), ic its own image's channels.
template <bool GRAD>
__device__ __forceinline__ UlData ul_data(const UlArgs& a, const UlSample& s, int x, int y, float fu, float fv, float oc,
                                          const float (&ic)[kUlMaxC]) {
  UlData r = {kUlNonfinite, 0.f, 0.f, 0.f};
  const float au = a.mult * fu, av = a.mult * fv;
  if (!finite_1e9(au) || !finite_1e9(av)) return r;
  if (!(oc == 0.0f)) {
    r.cls = kUlOccluded;
    return r;
  }
  const float x2 = (float)x + au, y2 = (float)y + av;
  if (!(x2 >= 0.f && y2 >= 0.f && x2 < (float)a.W && y2 < (float)a.H)) {
    r.cls = kUlOutside;
    return r;
  }
  const BilinearTaps t = bilinear_taps(x2, y2, a.W, a.H);
  const float gy = (float)t.iyB - y2, gx = (float)t.ixR - x2;
  const size_t hw = (size_t)a.H * a.W;
  float e = 0.f, su = 0.f, sv = 0.f;
  bool fin = true;
  for (int c = 0; c < a.C; ++c) {
    const float* __restrict__ p = s.Io + (size_t)c * hw;
    const float TL = p[t.oTL], TR = p[t.oTR], BL = p[t.oBL], BR = p[t.oBR], I = ic[c];
    fin = fin && finite_1e9(TL) && finite_1e9(TR) && finite_1e9(BL) && finite_1e9(BR) && finite_1e9(I);
    const float warped = ((t.wTL * TL + t.wTR * TR) + t.wBL * BL) + t.wBR * BR;
    const float d = I - warped;
    if constexpr (GRAD) {
      const float dp = ul_dpsi(d, a.eps_d, a.gam_d);
      const float tu = gy * (TR - TL) + (1.f - gy) * (BR - BL);
      const float tv = gx * (BL - TL) + (1.f - gx) * (BR - TR);
      su += dp * tu;
      sv += dp * tv;
    } else {
      e += ul_psi(d, a.eps_d, a.gam_d);
    }
  }
  if (!fin) return r;
  r.cls = kUlCounted;
  r.e = e; r.su = su; r.sv = sv;
  return r;
}

struct UlTerm {
  bool valid;
  float wgt, su, sv;
};

// The smoothness term owned by pixel (x, y), which is inside the plane, along (dx, dy) = (1, 0) or (0, 1).
__device__ __forceinline__ UlTerm ul_term(const UlArgs& a, const UlSample& s, int x, int y, int dx, int dy) {
  UlTerm t = {false, 1.f, 0.f, 0.f};
  const int xp = x + dx, yp = y + dy;
  if (xp >= a.W || yp >= a.H) return t;
  int xq = x, yq = y;
  if (a.order == 2) {
    xq = x - dx; yq = y - dy;
    if (xq < 0 || yq < 0) return t;
  }
  const int o0 = y * a.W + x, op = yp * a.W + xp, oq = yq * a.W + xq;
  const float u0 = a.mult * s.u[o0], v0 = a.mult * s.v[o0], up = a.mult * s.u[op], vp = a.mult * s.v[op];
  if (!finite_1e9(u0) || !finite_1e9(v0) || !finite_1e9(up) || !finite_1e9(vp)) return t;
  if (a.order == 2) {
    const float um = a.mult * s.u[oq], vm = a.mult * s.v[oq];
    if (!finite_1e9(um) || !finite_1e9(vm)) return t;
    t.su = (um - 2.0f * u0) + up;
    t.sv = (vm - 2.0f * v0) + vp;
  } else {
    t.su = up - u0;
    t.sv = vp - v0;
  }
  if (a.edge != 0.f) {
    const size_t hw = (size_t)a.H * a.W;
    float g = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float ip = s.Ia[(size_t)c * hw + op], iq = s.Ia[(size_t)c * hw + oq];
      if (!finite_1e9(ip) || !finite_1e9(iq)) return t;
      g += fabsf(ip - iq);
    }
    t.wgt = expf((-a.edge) * (g / (float)a.C));
  }
  t.valid = true;
  return t;
}

// h of the header for the term owned by (x, y): (wgt psi'(s_u), wgt psi'(s_v)), zeros where there is no such term
__device__ __forceinline__ void ul_h(const UlArgs& a, const UlSample& s, int x, int y, int dx, int dy, float& hu, float& hv) {
  hu = 0.f; hv = 0.f;
  if (x < 0 || y < 0 || x >= a.W || y >= a.H) return;
  const UlTerm t = ul_term(a, s, x, y, dx, dy);
  if (!t.valid) return;
  hu = t.wgt * ul_dpsi(t.su, a.eps_s, a.gam_s);
  hv = t.wgt * ul_dpsi(t.sv, a.eps_s, a.gam_s);
}

__device__ __forceinline__ void ul_g(const UlArgs& a, const UlSample& s, int x, int y, int dx, int dy, float& gu, float& gv) {
  float mu, mv, cu, cv;
  ul_h(a, s, x - dx, y - dy, dx, dy, mu, mv);
  ul_h(a, s, x, y, dx, dy, cu, cv);
  if (a.order == 2) {
    float pu, pv;
    ul_h(a, s, x + dx, y + dy, dx, dy, pu, pv);
    gu = (mu - 2.0f * cu) + pu;
    gv = (mv - 2.0f * cv) + pv;
  } else {
    gu = mu - cu;
    gv = mv - cv;
  }
}

__device__ __forceinline__ UlSample ul_sample(const UlArgs& a, int d, long long n) {
  const size_t hw = (size_t)a.H * a.W;
  UlSample s;
  s.u = a.flow[d] + (size_t)n * 2 * hw;
  s.v = s.u + hw;
  s.Ia = a.img[d] + (size_t)n * a.C * hw;
  s.Io = a.img[1 - d] + (size_t)n * a.C * hw;
  s.occ = a.occ[d] ? a.occ[d] + (size_t)n * hw : nullptr;
  return s;
}

// what one thread has seen; counts stay integers until the reduction (a thread sees fewer than 2^31 pixels)
struct UlSums {
  double data, smooth;
  int cnt[4];
  int pixels, terms;
};

__device__ __forceinline__ void ul_count(UlSums& t, int cls) {      // (no indexing by cls: the counts stay in registers)
#pragma unroll
  for (int c = 0; c < 4; ++c) t.cnt[c] += cls == c ? 1 : 0;
}

// A thread's sums -> the workgroup's partial row: wave64 shuffle tree, the four waves in order.  row -> partial[((d * N + n) * B + chunk) * K].
__device__ __forceinline__ void ul_reduce(const UlArgs& a, int d, long long n, int chunk, double (*lds)[kUlK], const UlSums& t) {
  double row[kUlK];
  row[FN2_UNSUP_LOSS_PIXELS] = (double)t.pixels;
  row[FN2_UNSUP_LOSS_COUNTED] = (double)t.cnt[kUlCounted];
  row[FN2_UNSUP_LOSS_OCCLUDED] = (double)t.cnt[kUlOccluded];
  row[FN2_UNSUP_LOSS_OUTSIDE] = (double)t.cnt[kUlOutside];
  row[FN2_UNSUP_LOSS_NONFINITE] = (double)t.cnt[kUlNonfinite];
  row[FN2_UNSUP_LOSS_DATA_SUM] = t.data;
  row[FN2_UNSUP_LOSS_SMOOTH_TERMS] = (double)t.terms;
  row[FN2_UNSUP_LOSS_SMOOTH_SUM] = t.smooth;
  reduce_row<kUlK, 0u>(row, lds, a.partial + (((size_t)d * a.N + n) * a.chunks + chunk) * kUlK);
}

// Chunk `chunk` of (direction d, sample n) on the one-pixel path: pixels chunk * 256 + thread, then every B * 256 further on; every term
// loads what it reads.  FWD: row -> partial[((d * N + n) * B + chunk) * K].  Otherwise the gradient of the chunk's pixels -> diff[d].
template <bool FWD>
__device__ __forceinline__ void ul_chunk1(const UlArgs& a, int d, long long n, int chunk, double (*lds)[kUlK], float kd, float ks) {
  const int W = a.W, H = a.H;
  const size_t hw = (size_t)H * W;
  const UlSample s = ul_sample(a, d, n);
  UlSums t = {};
  for (long long un = (long long)chunk * kThreads + threadIdx.x; un < (long long)hw; un += (long long)a.chunks * kThreads) {
    const unsigned r = (unsigned)un;                                       // H W < 2^30
    const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * W);
    float ic[kUlMaxC];
#pragma unroll
    for (int c = 0; c < kUlMaxC; ++c) ic[c] = c < a.C ? s.Ia[(size_t)c * hw + r] : 0.f;
    const UlData p = ul_data<!FWD>(a, s, x, y, s.u[r], s.v[r], s.occ ? s.occ[r] : 0.f, ic);
    if constexpr (FWD) {
      t.pixels += 1;
      ul_count(t, p.cls);
      if (p.cls == kUlCounted) t.data += (double)p.e;
      const UlTerm tx = ul_term(a, s, x, y, 1, 0);
      if (tx.valid) {
        t.terms += 1;
        t.smooth += (double)(tx.wgt * (ul_psi(tx.su, a.eps_s, a.gam_s) + ul_psi(tx.sv, a.eps_s, a.gam_s)));
      }
      const UlTerm ty = ul_term(a, s, x, y, 0, 1);
      if (ty.valid) {
        t.terms += 1;
        t.smooth += (double)(ty.wgt * (ul_psi(ty.su, a.eps_s, a.gam_s) + ul_psi(ty.sv, a.eps_s, a.gam_s)));
      }
    } else {
      float du = 0.f, dv = 0.f;
      if (p.cls == kUlCounted) {
        du = (-kd) * p.su;
        dv = (-kd) * p.sv;
      }
      float gxu, gxv, gyu, gyv;
      ul_g(a, s, x, y, 1, 0, gxu, gxv);
      ul_g(a, s, x, y, 0, 1, gyu, gyv);
      const float gu = gxu + gyu, gv = gxv + gyv;
      float* __restrict__ o = a.diff[d] + (size_t)n * 2 * hw + r;
      o[0] = a.mult * (du + ks * gu);
      o[hw] = a.mult * (dv + ks * gv);
    }
  }
  if constexpr (FWD) ul_reduce(a, d, n, chunk, lds, t);
}

// ---- the four-pixel path: the neighbourhood of a unit in registers --------------------------------------------------------------
// A unit is the pixels x .. x + 3 of row y.  Its smoothness terms read the flows (and, with an edge weight, the own image) of row y over
// x - 2 .. x + 5 and of the rows y - 2 .. y + 2 over x .. x + 3 (forward and first order: one row / column less on each side).  Those are
// loaded once as four-pixel accesses -- three for row y, one per other row -- and every term is evaluated once per thread: the x terms
// owned by x - 1 .. x + 4 serve all four pixels.  The arithmetic per term is that of ul_term, so the bits are those of the one-pixel path.

// N scaled flows along a line through the unit; bit i of ok: entry i is inside the plane and both its components are ok
template <int N>
struct UlLine {
  float u[N], v[N];
  unsigned ok;
};

// the term owned by entry i of a line: false where one of the entries it reads is missing or not finite
template <int N>
__device__ __forceinline__ bool ul_line_term(const UlArgs& a, const UlLine<N>& L, int i, float& su, float& sv) {
  const unsigned need = (1u << i) | (1u << (i + 1)) | (a.order == 2 ? 1u << (i - 1) : 0u);
  if ((L.ok & need) != need) return false;
  if (a.order == 2) {
    su = (L.u[i - 1] - 2.0f * L.u[i]) + L.u[i + 1];
    sv = (L.v[i - 1] - 2.0f * L.v[i]) + L.v[i + 1];
  } else {
    su = L.u[i + 1] - L.u[i];
    sv = L.v[i + 1] - L.v[i];
  }
  return true;
}

// one channel's part of the edge weight of the term owned by entry i of a line of image values: g += |I(p+) - I(q)|; false where one of
// the two is not finite (entries outside the plane hold 0: their terms are dropped by the flows' ok bits)
template <int N>
__device__ __forceinline__ bool ul_line_edge(const UlArgs& a, const float (&I)[N], int i, float& g) {
  const float ip = I[i + 1], iq = a.order == 2 ? I[i - 1] : I[i];
  g += fabsf(ip - iq);
  return finite_1e9(ip) && finite_1e9(iq);
}

// four values at p where `there`, else zeros
template <bool VEC>
__device__ __forceinline__ void ul_load4_if(bool there, const float* __restrict__ p, float* o) {
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  if (there) load<4, VEC>(p, t);
  o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
}

template <bool VEC, bool FWD>
__device__ __forceinline__ void ul_unit4(const UlArgs& a, const UlSample& s, int d, long long n, unsigned r, UlSums& t, float kd, float ks) {
  const int W = a.W, H = a.H;
  const size_t hw = (size_t)H * W;
  const int y = (int)(r / (unsigned)W), x = (int)(r - (unsigned)y * W);      // W % 4 == 0, so x % 4 == 0 and x + 3 < W
  const bool edge = a.edge != 0.f;
  const bool left = x >= 4, right = x + 4 < W;
  // rows y - 2, y - 1, y + 1, y + 2: inside the plane and read by a term
  const int reach = (!FWD && a.order == 2) ? 2 : 1;
  const int dys[4] = {-2, -1, 1, 2};
  bool there[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) there[q] = abs(dys[q]) <= reach && y + dys[q] >= 0 && y + dys[q] < H && !(FWD && a.order == 1 && dys[q] < 0);
  constexpr int XO = FWD ? 4 : 3, XN = FWD ? 4 : 6;      // the x terms evaluated: owners row[XO] .. row[XO + XN - 1]
  constexpr int YO = FWD ? 2 : 1, YN = FWD ? 1 : 3;      // the y terms evaluated per pixel: owners col[YO] .. col[YO + YN - 1]

  UlLine<12> row;
  UlLine<5> col[4];
  float fu[4], fv[4];                                       // the unit's own raw flows
  {
    float ru[12], rv[12];
    ul_load4_if<VEC>(left, s.u + r - 4, ru);
    ul_load4_if<VEC>(left, s.v + r - 4, rv);
    ul_load4_if<VEC>(true, s.u + r, ru + 4);
    ul_load4_if<VEC>(true, s.v + r, rv + 4);
    ul_load4_if<VEC>(right, s.u + r + 4, ru + 8);
    ul_load4_if<VEC>(right, s.v + r + 4, rv + 8);
    const unsigned in = 0x0F0u | (left ? 0x00Fu : 0u) | (right ? 0xF00u : 0u);
    row.ok = 0;
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      row.u[j] = a.mult * ru[j];
      row.v[j] = a.mult * rv[j];
      if (((in >> j) & 1u) && finite_1e9(row.u[j]) && finite_1e9(row.v[j])) row.ok |= 1u << j;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      fu[k] = ru[4 + k]; fv[k] = rv[4 + k];
      col[k].u[2] = row.u[4 + k]; col[k].v[2] = row.v[4 + k];
      col[k].ok = ((row.ok >> (4 + k)) & 1u) << 2;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = dys[q] + 2;
      float cu[4], cv[4];
      const long long off = (long long)dys[q] * W;
      ul_load4_if<VEC>(there[q], s.u + r + off, cu);
      ul_load4_if<VEC>(there[q], s.v + r + off, cv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        col[k].u[e] = a.mult * cu[k];
        col[k].v[e] = a.mult * cv[k];
        if (there[q] && finite_1e9(col[k].u[e]) && finite_1e9(col[k].v[e])) col[k].ok |= 1u << e;
      }
    }
  }
  float oc[4];
  if (s.occ) {
    load<4, VEC>(s.occ + r, oc);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) oc[k] = 0.f;
  }
  // the own image: the unit's pixels for the data term and, with an edge weight, the neighbourhood, one channel at a time
  float ic[kUlMaxC][4];
  float gx[XN], gy[4][YN];
  unsigned xfin = 0xFFFFFFFFu, yfin = 0xFFFFFFFFu;           // bit t (bit k * YN + t): every image value of that term is finite so far
#pragma unroll
  for (int t2 = 0; t2 < XN; ++t2) gx[t2] = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t2 = 0; t2 < YN; ++t2) gy[k][t2] = 0.f;
#pragma unroll
  for (int c = 0; c < kUlMaxC; ++c) {
    if (c < a.C) {
      const float* __restrict__ p = s.Ia + (size_t)c * hw + r;
      if (!edge) {
        load<4, VEC>(p, ic[c]);
      } else {
        float ir[12], icol[5];
        ul_load4_if<VEC>(left, p - 4, ir);
        ul_load4_if<VEC>(true, p, ir + 4);
        ul_load4_if<VEC>(right, p + 4, ir + 8);
        float rows[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ul_load4_if<VEC>(there[q], p + (long long)dys[q] * W, rows[q]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ic[c][k] = ir[4 + k];
#pragma unroll
        for (int t2 = 0; t2 < XN; ++t2)
          if (!ul_line_edge<12>(a, ir, XO + t2, gx[t2])) xfin &= ~(1u << t2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          icol[0] = rows[0][k]; icol[1] = rows[1][k]; icol[2] = ir[4 + k]; icol[3] = rows[2][k]; icol[4] = rows[3][k];
#pragma unroll
          for (int t2 = 0; t2 < YN; ++t2)
            if (!ul_line_edge<5>(a, icol, YO + t2, gy[k][t2])) yfin &= ~(1u << (k * YN + t2));
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) ic[c][k] = 0.f;
    }
  }
  // the terms: FWD their values (x then y per pixel), else h = wgt psi' per component
  float xa[XN], xb[XN], ya[4][YN], yb[4][YN];
  bool xv[XN], yv[4][YN];
#pragma unroll
  for (int t2 = 0; t2 < XN; ++t2) {
    float su = 0.f, sv = 0.f;
    const bool wanted = FWD || a.order == 2 || t2 < XN - 1;              // first-order backward: the owner x + 4 reaches no pixel of the unit
    xv[t2] = wanted && ul_line_term<12>(a, row, XO + t2, su, sv) && (!edge || ((xfin >> t2) & 1u));
    xa[t2] = 0.f; xb[t2] = 0.f;
    if (xv[t2]) {
      const float wgt = edge ? expf((-a.edge) * (gx[t2] / (float)a.C)) : 1.f;
      if constexpr (FWD) {
        xa[t2] = wgt * (ul_psi(su, a.eps_s, a.gam_s) + ul_psi(sv, a.eps_s, a.gam_s));
      } else {
        xa[t2] = wgt * ul_dpsi(su, a.eps_s, a.gam_s);
        xb[t2] = wgt * ul_dpsi(sv, a.eps_s, a.gam_s);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int t2 = 0; t2 < YN; ++t2) {
      float su = 0.f, sv = 0.f;
      const bool wanted = FWD || a.order == 2 || t2 < YN - 1;
      yv[k][t2] = wanted && ul_line_term<5>(a, col[k], YO + t2, su, sv) && (!edge || ((yfin >> (k * YN + t2)) & 1u));
      ya[k][t2] = 0.f; yb[k][t2] = 0.f;
      if (yv[k][t2]) {
        const float wgt = edge ? expf((-a.edge) * (gy[k][t2] / (float)a.C)) : 1.f;
        if constexpr (FWD) {
          ya[k][t2] = wgt * (ul_psi(su, a.eps_s, a.gam_s) + ul_psi(sv, a.eps_s, a.gam_s));
        } else {
          ya[k][t2] = wgt * ul_dpsi(su, a.eps_s, a.gam_s);
          yb[k][t2] = wgt * ul_dpsi(sv, a.eps_s, a.gam_s);
        }
      }
    }
  float ou[4], ov[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float ick[kUlMaxC] = {ic[0][k], ic[1][k], ic[2][k], ic[3][k]};
    const UlData p = ul_data<!FWD>(a, s, x + k, y, fu[k], fv[k], oc[k], ick);
    if constexpr (FWD) {
      t.pixels += 1;
      ul_count(t, p.cls);
      if (p.cls == kUlCounted) t.data += (double)p.e;
      if (xv[k]) {
        t.terms += 1;
        t.smooth += (double)xa[k];
      }
      if (yv[k][0]) {
        t.terms += 1;
        t.smooth += (double)ya[k][0];
      }
    } else {
      float du = 0.f, dv = 0.f;
      if (p.cls == kUlCounted) {
        du = (-kd) * p.su;
        dv = (-kd) * p.sv;
      }
      float gxu, gxv, gyu, gyv;
      if (a.order == 2) {
        gxu = (xa[k] - 2.0f * xa[k + 1]) + xa[k + 2];
        gxv = (xb[k] - 2.0f * xb[k + 1]) + xb[k + 2];
        gyu = (ya[k][0] - 2.0f * ya[k][1]) + ya[k][YN - 1];
        gyv = (yb[k][0] - 2.0f * yb[k][1]) + yb[k][YN - 1];
      } else {
        gxu = xa[k] - xa[k + 1];
        gxv = xb[k] - xb[k + 1];
        gyu = ya[k][0] - ya[k][YN > 1 ? 1 : 0];
        gyv = yb[k][0] - yb[k][YN > 1 ? 1 : 0];
      }
      const float gu = gxu + gyu, gv = gxv + gyv;
      ou[k] = a.mult * (du + ks * gu);
      ov[k] = a.mult * (dv + ks * gv);
    }
  }
  if constexpr (!FWD) {
    float* __restrict__ o = a.diff[d] + (size_t)n * 2 * hw + r;
    store<4, VEC>(o, ou);
    store<4, VEC>(o + hw, ov);
  }
}

// Chunk `chunk` of (direction d, sample n) on the four-pixel path: units chunk * 256 + thread, then every B * 256 further on.
template <bool VEC, bool FWD>
__device__ __forceinline__ void ul_chunk4(const UlArgs& a, int d, long long n, int chunk, double (*lds)[kUlK], float kd, float ks) {
  const long long units = (long long)(((size_t)a.H * a.W) / 4);
  const UlSample s = ul_sample(a, d, n);
  UlSums t = {};
  for (long long un = (long long)chunk * kThreads + threadIdx.x; un < units; un += (long long)a.chunks * kThreads)
    ul_unit4<VEC, FWD>(a, s, d, n, (unsigned)un * 4u, t, kd, ks);                // H W < 2^30
  if constexpr (FWD) ul_reduce(a, d, n, chunk, lds, t);
}

template <bool FWD>
__device__ __forceinline__ void ul_items(const UlArgs& a, double (*lds)[kUlK]) {
  const long long per_dir = (long long)a.N * a.chunks;
  for (long long w = blockIdx.x; w < a.dirs * per_dir; w += gridDim.x) {
    const int d = w >= per_dir ? 1 : 0;
    const long long i = w - d * per_dir;
    const long long n = i / a.chunks;
    const int chunk = (int)(i % a.chunks);
    float kd = 0.f, ks = 0.f;
    if constexpr (!FWD) {
      const double* __restrict__ tot = a.totals + ((size_t)d * (a.N + 1) + a.N) * kUlK;
      const float gdiff = a.total_diff ? a.total_diff[0] : 1.f;
      kd = gdiff * (float)((double)a.dw / fmax(tot[FN2_UNSUP_LOSS_COUNTED], 1.0));
      ks = gdiff * (float)((double)a.sw / fmax(tot[FN2_UNSUP_LOSS_SMOOTH_TERMS], 1.0));
    }
    if (!a.quad) ul_chunk1<FWD>(a, d, n, chunk, lds, kd, ks);
    else if (a.vec) ul_chunk4<true, FWD>(a, d, n, chunk, lds, kd, ks);
    else ul_chunk4<false, FWD>(a, d, n, chunk, lds, kd, ks);
  }
}

__global__ void __launch_bounds__(kThreads) unsup_loss_partial(UlArgs a) {
  __shared__ double lds[4][kUlK];
  ul_items<true>(a, lds);
}

__global__ void __launch_bounds__(kThreads) unsup_loss_grad(UlArgs a) {
  ul_items<false>(a, nullptr);
}

// One workgroup.  The two directions are the groups of the plain finalise, a direction that was not run gets zeros; then one thread
// forms the loss.
__global__ void __launch_bounds__(kThreads) unsup_loss_final(UlArgs a) {
  finalize_rows<kUlK, 0u>(a.partial, a.results, 2, a.N, a.chunks, a.dirs);
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0 && a.loss) {
    double L = 0.0;
    for (int d = 0; d < a.dirs; ++d) {
      const double* t = a.results + ((size_t)d * (a.N + 1) + a.N) * kUlK;
      const double dterm = ((double)a.dw * t[FN2_UNSUP_LOSS_DATA_SUM]) / fmax(t[FN2_UNSUP_LOSS_COUNTED], 1.0);
      const double sterm = ((double)a.sw * t[FN2_UNSUP_LOSS_SMOOTH_SUM]) / fmax(t[FN2_UNSUP_LOSS_SMOOTH_TERMS], 1.0);
      L = L + (dterm + sterm);
    }
    a.loss[0] = (float)L;
  }
}

static int ul_shape(const char* what, int N, int C, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return fail(FN2_ERR_INVALID_ARG, "%s: bad shape [%d,%d,%d,%d]", what, N, C, H, W);
  if (C < 1 || C > kUlMaxC) return fail(FN2_ERR_INVALID_ARG, "%s: C = %d channels (need 1 .. %d)", what, C, kUlMaxC);
  return check_planes(what, N, C > 2 ? C : 2, H, W);      // the larger of an image [N,C,H,W] and a flow [N,2,H,W]
}

static size_t ul_ws_bytes(int N, int H, int W) { return sizeof(double) * kUlK * 2 * (size_t)N * chunks((long long)H * W); }

// the checks both directions of differentiation share; fills what they share of `a`
static int ul_setup(const char* what, UlArgs& a, const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw,
                    const float* occ_bw, int N, int C, int H, int W, float data_weight, float smooth_weight, float eps_d, float gamma_d,
                    float eps_s, float gamma_s, float edge_weight, int smooth_order, float flow_mult) {
  if (!img0) return fail(FN2_ERR_INVALID_ARG, "%s: img0 == NULL", what);
  if (!img1) return fail(FN2_ERR_INVALID_ARG, "%s: img1 == NULL", what);
  if (!fw) return fail(FN2_ERR_INVALID_ARG, "%s: fw == NULL", what);
  int rc = ul_shape(what, N, C, H, W);
  if (rc) return rc;
  const float nonneg[5] = {data_weight, smooth_weight, eps_d, eps_s, edge_weight};
  const char* nonneg_names[5] = {"data_weight", "smooth_weight", "eps_d", "eps_s", "edge_weight"};
  for (int k = 0; k < 5; ++k)
    if (!(nonneg[k] >= 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: %s = %g (need >= 0)", what, nonneg_names[k], nonneg[k]);
  if (!(gamma_d > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: gamma_d = %g (need > 0)", what, gamma_d);
  if (!(gamma_s > 0.f)) return fail(FN2_ERR_INVALID_ARG, "%s: gamma_s = %g (need > 0)", what, gamma_s);
  if (smooth_order != 1 && smooth_order != 2) return fail(FN2_ERR_INVALID_ARG, "%s: smooth_order = %d (need 1 or 2)", what, smooth_order);
  if (flow_mult != flow_mult) return fail(FN2_ERR_INVALID_ARG, "%s: flow_mult is NaN", what);
  a = UlArgs{};
  a.img[0] = img0; a.img[1] = img1;
  a.flow[0] = fw; a.flow[1] = bw;
  a.occ[0] = occ_fw; a.occ[1] = occ_bw;
  a.N = N; a.C = C; a.H = H; a.W = W;
  a.chunks = chunks((long long)H * W);
  a.dirs = bw ? 2 : 1;
  a.quad = (W % 4) == 0;
  a.vec = a.quad && aligned16(img0) && aligned16(img1) && aligned16(fw) && aligned16(bw) && aligned16(occ_fw) &&
          aligned16(occ_bw);
  a.order = smooth_order;
  a.dw = data_weight; a.sw = smooth_weight; a.eps_d = eps_d; a.gam_d = gamma_d; a.eps_s = eps_s; a.gam_s = gamma_s;
  a.edge = edge_weight; a.mult = flow_mult;
  return FN2_OK;
}

}  // namespace fn2

using namespace fn2;

FN2_API int fn2_unsup_loss_sizes(int N, int H, int W, size_t* workspace_bytes, int* K) {
  int rc = ul_shape("unsup_loss_sizes", N, 1, H, W);
  if (rc) return rc;
  if (workspace_bytes) *workspace_bytes = ul_ws_bytes(N, H, W);
  if (K) *K = kUlK;
  return FN2_OK;
}

FN2_API int fn2_unsup_loss_forward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw,
                                   const float* occ_bw, int N, int C, int H, int W, float data_weight, float smooth_weight, float eps_d,
                                   float gamma_d, float eps_s, float gamma_s, float edge_weight, int smooth_order, float flow_mult,
                                   double* results, float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "unsup_loss_forward";
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  UlArgs a;
  int rc = ul_setup(what, a, img0, img1, fw, bw, occ_fw, occ_bw, N, C, H, W, data_weight, smooth_weight, eps_d, gamma_d, eps_s, gamma_s,
                    edge_weight, smooth_order, flow_mult);
  if (rc) return rc;
  if (!workspace || workspace_bytes < ul_ws_bytes(N, H, W))
    return fail(FN2_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu)", what, workspace ? workspace_bytes : (size_t)0, ul_ws_bytes(N, H, W));
  a.partial = reinterpret_cast<double*>(workspace);
  a.results = results;
  a.loss = loss;
  const long long items = (long long)a.dirs * N * a.chunks;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(unsup_loss_partial, grid_for(items), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(unsup_loss_final, dim3(1), dim3(kThreads), 0, st, a);
  return check_launch(what);
}

FN2_API int fn2_unsup_loss_backward(const float* img0, const float* img1, const float* fw, const float* bw, const float* occ_fw,
                                    const float* occ_bw, int N, int C, int H, int W, float data_weight, float smooth_weight, float eps_d,
                                    float gamma_d, float eps_s, float gamma_s, float edge_weight, int smooth_order, float flow_mult,
                                    const double* results, const float* total_diff, float* fw_diff, float* bw_diff, void* stream) {
  const char* what = "unsup_loss_backward";
  if (!results) return fail(FN2_ERR_INVALID_ARG, "%s: results == NULL", what);
  if (!fw_diff) return fail(FN2_ERR_INVALID_ARG, "%s: fw_diff == NULL", what);
  if (bw_diff && !bw) return fail(FN2_ERR_INVALID_ARG, "%s: bw_diff without a bw", what);
  UlArgs a;
  int rc = ul_setup(what, a, img0, img1, fw, bw, occ_fw, occ_bw, N, C, H, W, data_weight, smooth_weight, eps_d, gamma_d, eps_s, gamma_s,
                    edge_weight, smooth_order, flow_mult);
  if (rc) return rc;
  a.totals = results;
  a.total_diff = total_diff;
  a.diff[0] = fw_diff; a.diff[1] = bw_diff;
  a.dirs = bw_diff ? 2 : 1;
  a.vec = a.vec && aligned16(fw_diff) && aligned16(bw_diff);
  const long long items = (long long)a.dirs * N * a.chunks;
  hipLaunchKernelGGL(unsup_loss_grad, grid_for(items), dim3(kThreads), 0, as_stream(stream), a);
  return check_launch(what);
}
