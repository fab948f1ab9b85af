// General-geometry Convolution / Deconvolution on v_mfma_f32_16x16x4_f32 (exact fp32): the last resort behind the specialised families.
// Contract, operand layout and summation order: include/flownet2_hip_conv_general.h (square taps, fn2_conv_desc) and
// include/flownet2_hip_conv_geometry.h (rectangular taps, per-axis stride / pad / dilation, groups: the same code, widened) and
// include/flownet2_hip_conv_volume.h (a depth axis in front of the two: one more digit of the same pixel and k-row numbers).
//
// Everything is stated on the two SIDES of the layer, the larger map L and the smaller map S (Convolution: L = bottom, S = top;
// Deconvolution: L = top, S = bottom).  The weight blob is [Cs][Cl / group][kh][kw] for both kinds.  Per group (channels Clg = Cl / group,
// Csg = Cs / group, the slices [g Clg, ...) and [g Csg, ...) of the two blobs, the rows [g Csg, ...) of the weight blob)
//   forward gather    L -> S   Convolution forward, Deconvolution data gradient      M = Csg, K = Clg kh kw, Wp[cs][(cl, tap)] = W[cs][cl][tap]
//   transposed gather S -> L   Convolution data gradient, Deconvolution forward      M = Clg, K = Csg kh kw, Wp[cl][(cs, tap)] = W[cs][cl][tap]
//   weight gradient            dW[cs][(cl, tap)] = sum over (n, S pixels) of S[cs][p] x (forward gather of L)[(cl, tap)][p]
// so there are two gather kernels (one template), two pack layouts and one weight-gradient kernel for the four layer uses.  The group is a
// grid factor.  Every kernel that gathers exists three times, by the template parameter GEO: kPlain is the plain geometry (square taps, one
// stride, one pad, dilation 1, group 1), where the per-axis values, the dilation products and the group offsets compile away; kGen is every
// other geometry with two spatial axes; kVol adds the depth axis (pixels (z, y, x), k-rows (c, kz, ky, kx)) and is run only where the depth
// axis is not trivial.  All run the same accumulation chain per output value.
//
// Tiles.  A workgroup is 4 waves.  Gather kernel: 64 consecutive pixels (flattened y Wout + x, so a tile may wrap rows) of one sample x
// NG = 1, 2 or 4 groups of 16 output channels (by the channel count alone); per chunk of 16 k-rows every thread gathers 4 values (its
// pixel, k-rows wave, wave + 4, ...: the k decomposition is wave-uniform and advanced by carries, the divisions by the stride and the
// map width are multiplications), the next chunk's loads are in flight while the MFMAs of this one run; wave w multiplies pixels 16 w ..
// 16 w + 15 with the NG groups (the last block's missing groups repeat the last real one and are not stored).  Weight gradient: 16 k-columns x
// 64 channels, wave w owns channel group w, the reduction runs over chunks of 64 pixels staged the same way.
#include "mfma_tile.hpp"

#include "../../include/flownet2_hip_conv_general.h"
#include "../../include/flownet2_hip_conv_geometry.h"
#include "../../include/flownet2_hip_conv_volume.h"

namespace fn2 {
namespace {

using mfma::f32x4;

constexpr int kPix = 64;        // pixels per tile / chunk
constexpr int kKC = 16;         // k-rows per chunk (four k-steps)
constexpr int kThreads = 256;
constexpr int kColStrideG = 80; // LDS row stride of the col tile, gather kernels: == 16 (mod 32), the k-step read [4 rows][16 pixels] is conflict-free
constexpr int kColStrideW = 66; // weight gradient: == 2 (mod 32), the read [16 rows][4 pixels] is conflict-free
constexpr long long kMaxElems = 0x7fffffffll;
constexpr long long kMaxTiles = 0x3fffff00ll;

// ------------------------------------------------------------------------------------------------ host geometry
enum Geo { kPlain = 0, kGen = 1, kVol = 2 };      // the geometry template parameter of the gathering kernels

struct Sides {
  int N, Cl, Dl, Hl, Wl, Cs, Ds, Hs, Ws, kd, kh, kw, sd, sh, sw, pd, ph, pw, dd, dh, dw, group;
  int Cin, Cout;            // the layer's own names of the two channel counts (the slices of bottom and top)
  bool plain;               // two spatial axes, square taps, one stride, one pad, dilation 1, group 1: the kPlain kernels
  bool volume;              // a depth axis that is not trivial (not Din = kd = sd = dd = 1, pd = 0): the kVol kernels
  long long Pl() const { return (long long)Dl * Hl * Wl; }      // voxels of the two maps
  long long Ps() const { return (long long)Ds * Hs * Ws; }
  int taps() const { return kd * kh * kw; }
};

// the 19 ints of include/flownet2_hip_conv_volume.h: what every entry point is stated on
enum { kGN, kGCin, kGDin, kGHin, kGWin, kGCout, kGkd, kGkh, kGkw, kGsd, kGsh, kGsw, kGpd, kGph, kGpw, kGdd, kGdh, kGdw, kGgroup, kGeomInts };

// a caller's geometry as the 19 ints: the 19 themselves, or the 14 of include/flownet2_hip_conv_geometry.h with a trivial depth axis
struct Geom {
  int v[kGeomInts];
  bool null, depth;         // depth: stated with a depth axis (what a refusal prints)
  Geom() : null(true), depth(false) {}
  static Geom from_volume(const int* w) {
    Geom g;
    g.null = !w; g.depth = true;
    if (w) for (int i = 0; i < kGeomInts; ++i) g.v[i] = w[i];
    return g;
  }
  static Geom from_planar(const int* w) {       // {N, Cin, Hin, Win, Cout, kh, kw, sh, sw, ph, pw, dh, dw, group}
    Geom g;
    g.null = !w;
    if (w) {
      const int u[kGeomInts] = {w[0], w[1], 1, w[2], w[3], w[4], 1, w[5], w[6], 1, w[7], w[8], 0, w[9], w[10], 1, w[11], w[12], w[13]};
      for (int i = 0; i < kGeomInts; ++i) g.v[i] = u[i];
    }
    return g;
  }
  // fn2_conv_desc: (k, k, s, s, p, p, 1, 1, 1)
  static Geom from_desc(const fn2_conv_desc* d) {
    if (!d) return Geom();
    const int w[14] = {d->N, d->Cin, d->Hin, d->Win, d->Cout, d->kernel, d->kernel, d->stride, d->stride, d->pad, d->pad, 1, 1, 1};
    return from_planar(w);
  }
};

inline long long cdivll(long long a, long long b) { return (a + b - 1) / b; }

// a b c where every partial product has to stay inside the 32-bit element limit; false: it does not
inline bool mul3(long long a, long long b, long long c, long long& out) {
  out = a * b;              // a, b, c <= kMaxElems: no long long overflow in either step
  if (out > kMaxElems) return false;
  out *= c;
  return out <= kMaxElems;
}

// the geometry on its two sides; false: invalid, output extent below 1, or a blob beyond the 32-bit index limits
bool make_sides(const Geom& geom, int transposed, Sides& g) {
  if (geom.null) return false;
  const int* v = geom.v;
  for (int i = 0; i < kGeomInts; ++i)
    if (v[i] < ((i >= kGpd && i <= kGpw) ? 0 : 1)) return false;      // pad >= 0, everything else >= 1
  if (v[kGCin] % v[kGgroup] != 0 || v[kGCout] % v[kGgroup] != 0) return false;
  // per axis (depth, height, width): the dilated extent of the taps and the top extent
  long long ext[3], out[3];
  for (int a = 0; a < 3; ++a) {
    const long long in = v[kGDin + a], k = v[kGkd + a], s = v[kGsd + a], p = v[kGpd + a], d = v[kGdd + a];
    ext[a] = d * (k - 1) + 1;
    if (ext[a] > kMaxElems) return false;
    if (!transposed) {
      if (in + 2 * p < ext[a]) return false;
      out[a] = (in + 2 * p - ext[a]) / s + 1;
    } else {
      out[a] = s * (in - 1) + ext[a] - 2 * p;
    }
    if (out[a] < 1 || out[a] > kMaxElems) return false;
  }
  long long kk, pb, pt;
  if (!mul3(v[kGkd], v[kGkh], v[kGkw], kk) || !mul3(v[kGDin], v[kGHin], v[kGWin], pb) || !mul3(out[0], out[1], out[2], pt)) return false;
  const long long bottom = (long long)v[kGN] * v[kGCin], top = (long long)v[kGN] * v[kGCout];
  if (bottom > kMaxElems || top > kMaxElems) return false;
  if (bottom * pb > kMaxElems || top * pt > kMaxElems) return false;
  const long long cc = (long long)v[kGCin] * (v[kGCout] / v[kGgroup]);
  if (cc > kMaxElems || cc * kk > kMaxElems) return false;
  // the padded operands: group x (channels of a group rounded to 16) x (K of a group rounded to 16)
  const long long cmax = (v[kGCin] > v[kGCout] ? v[kGCin] : v[kGCout]) / v[kGgroup];
  if (v[kGgroup] * (cdivll(cmax, 16) * 16) * (cdivll(cmax * kk, kKC) * kKC + kKC) > kMaxElems) return false;
  g.N = v[kGN]; g.kd = v[kGkd]; g.kh = v[kGkh]; g.kw = v[kGkw]; g.sd = v[kGsd]; g.sh = v[kGsh]; g.sw = v[kGsw]; g.pd = v[kGpd]; g.ph = v[kGph];
  g.pw = v[kGpw]; g.dd = v[kGdd]; g.dh = v[kGdh]; g.dw = v[kGdw];
  g.group = v[kGgroup]; g.Cin = v[kGCin]; g.Cout = v[kGCout];
  g.volume = !(v[kGDin] == 1 && g.kd == 1 && g.sd == 1 && g.pd == 0 && g.dd == 1);
  g.plain = !g.volume && g.kh == g.kw && g.sh == g.sw && g.ph == g.pw && g.dh == 1 && g.dw == 1 && g.group == 1;
  if (!transposed) {
    g.Cl = v[kGCin]; g.Dl = v[kGDin]; g.Hl = v[kGHin]; g.Wl = v[kGWin]; g.Cs = v[kGCout]; g.Ds = (int)out[0]; g.Hs = (int)out[1]; g.Ws = (int)out[2];
  } else {
    g.Cs = v[kGCin]; g.Ds = v[kGDin]; g.Hs = v[kGHin]; g.Ws = v[kGWin]; g.Cl = v[kGCout]; g.Dl = (int)out[0]; g.Hl = (int)out[1]; g.Wl = (int)out[2];
  }
  // the gathers' coordinates (y stride - pad + ky dilation and y + pad - ky dilation over the larger map) stay inside int
  if ((long long)g.Dl + 2ll * g.pd + ext[0] > kMaxElems || (long long)g.Hl + 2ll * g.ph + ext[1] > kMaxElems ||
      (long long)g.Wl + 2ll * g.pw + ext[2] > kMaxElems)
    return false;
  return true;
}

// one GEMM view of ONE group: M output channels, R reduction channels (K = R kh kw)
struct Gemm {
  int M, R, G, ksteps;      // G: 16-channel row groups; ksteps: k-steps of the padded K (a multiple of 4)
  long long K, Kpad;
};

Gemm make_gemm(int M, int R, int taps) {
  Gemm m;
  m.M = M; m.R = R; m.G = (M + 15) / 16;
  m.K = (long long)R * taps;
  m.Kpad = cdivll(m.K, kKC) * kKC;
  m.ksteps = (int)(m.Kpad / 4);
  return m;
}

// which gather serves pass 0 (forward) / 1 (data gradient) of the layer kind: true = the transposed gather
inline bool pass_is_tr(int transposed, int pass) { return (pass == 1) != (transposed != 0); }
inline Gemm pass_gemm(const Sides& g, bool tr) {
  const int cl = g.Cl / g.group, cs = g.Cs / g.group;
  return tr ? make_gemm(cl, cs, g.taps()) : make_gemm(cs, cl, g.taps());
}
inline size_t packed_floats(const Sides& g, const Gemm& m) { return (size_t)g.group * (size_t)m.G * (size_t)m.ksteps * 64; }

struct WgradPlan {
  Gemm m;                   // M = Csg, R = Clg
  int ptiles, nsplit;       // 64-pixel chunks per sample; parts of the reduction
  long long chunks, per_part, tiles;
  size_t workspace_bytes;
};

WgradPlan make_wgrad(const Sides& g) {
  WgradPlan p;
  p.m = pass_gemm(g, false);
  p.ptiles = (int)cdivll(g.Ps(), kPix);
  p.chunks = (long long)g.N * p.ptiles;
  const long long out_tiles = (p.m.Kpad / kKC) * ((p.m.G + 3) / 4) * g.group;       // a 64-channel tile stays inside one group
  long long want = 2048 / out_tiles;                   // enough workgroups for the chip when the output has few tiles
  if (want > 64) want = 64;
  if (want > p.chunks) want = p.chunks;
  if (want < 1) want = 1;
  p.per_part = cdivll(p.chunks, want);
  p.nsplit = (int)cdivll(p.chunks, p.per_part);      // no empty part
  p.tiles = out_tiles * p.nsplit;
  p.workspace_bytes = sizeof(float) * (size_t)p.nsplit * (size_t)g.group * (size_t)(16 * p.m.G) * (size_t)p.m.Kpad;
  return p;
}

// 16-channel row groups per workgroup of the gather kernels: the three instantiations run the same accumulation chain per output value (the
// same bits); which one runs is a function of the channel count alone -- no autotuning -- unless the debug hook forces one
int& forced_groups() { static int f = 0; return f; }
inline int natural_groups(int G) { return G <= 1 ? 1 : G <= 2 ? 2 : 4; }
inline int groups_per_block(int G) { return forced_groups() ? forced_groups() : natural_groups(G); }

long long gather_tiles(const Sides& g, bool tr, const Gemm& m, int ng) {
  const long long P = tr ? g.Pl() : g.Ps();
  return (long long)g.N * cdivll(P, kPix) * cdivll(m.G, ng) * g.group;
}

bool supported(const Geom& geom, int transposed, Sides& g) {
  if (!make_sides(geom, transposed, g)) return false;
  const Gemm mf = pass_gemm(g, false), mt = pass_gemm(g, true);
  if (gather_tiles(g, false, mf, natural_groups(mf.G)) > kMaxTiles || gather_tiles(g, true, mt, natural_groups(mt.G)) > kMaxTiles) return false;
  const WgradPlan w = make_wgrad(g);
  return w.tiles <= kMaxTiles && w.workspace_bytes / sizeof(float) <= (size_t)kMaxElems;
}

// ------------------------------------------------------------------------------------------------ device: the col gather
struct GatherSrc {
  const float* in;          // channel c0 of sample 0 of the input blob
  int ctot, C, IH, IW;      // channels of the blob / of the slice, input map
  int OW;                   // width of the pixel space the tile runs over
  long long OP;             // its pixels (voxels)
  int kh, sh, ph;               // kPlain reads these alone, for both axes ...
  unsigned ow_magic, sh_magic;  // div_magic(OW), div_magic(sh)
  int kw, sw, pw, dh, dw;       // ... kGen these too ...
  int group;                    // the input channels of group g are [g C, (g + 1) C) from `in`
  unsigned sw_magic;            // div_magic(sw)
};

// ... and kVol the depth axis as well.  A structure of its own at the END of the kernels' arguments: what the other instantiations read lies
// where it lay before there was a depth axis
struct GatherDepth {
  int ID, OHW, kd, sd, pd, dd;      // input depth, pixels of one output plane, the depth axis of the taps
  unsigned ohw_magic, sd_magic;     // div_magic(OHW), div_magic(sd)
};

// n / d for 0 <= n < 2^32 without an integer division: with m = div_magic(d) = floor((2^32 - 1) / d), umulhi(n, m) is the quotient or one
// below it (m d = 2^32 - e with 1 <= e <= d, so n m / 2^32 lies in (n / d - 1, n / d]); one correction step makes it exact
inline unsigned div_magic(int d) { return 0xffffffffu / (unsigned)d; }

__device__ __forceinline__ void divmod(unsigned n, unsigned d, unsigned magic, unsigned& q, unsigned& r) {
  q = __umulhi(n, magic);
  r = n - q * d;
  if (r >= d) { ++q; r -= d; }
}

// the pixel of a thread in its tile, as the gather needs it: forward (y sh - ph, x sw - pw), transposed (y + ph, x + pw); kVol: z alike
struct PixelBase { int bz, by, bx; bool valid; };

template <bool TR, int GEO>
__device__ __forceinline__ PixelBase pixel_base(const GatherSrc& a, const GatherDepth& z, long long p) {
  constexpr bool GEN = GEO != kPlain;
  PixelBase b;
  b.valid = p < a.OP;
  unsigned up = b.valid ? (unsigned)p : 0u, uy, ux;
  b.bz = 0;
  if constexpr (GEO == kVol) {
    unsigned uz;
    divmod(up, (unsigned)z.OHW, z.ohw_magic, uz, up);
    b.bz = TR ? (int)uz + z.pd : (int)uz * z.sd - z.pd;
  }
  divmod(up, (unsigned)a.OW, a.ow_magic, uy, ux);
  const int y = (int)uy, x = (int)ux;
  const int sw = GEN ? a.sw : a.sh, pw = GEN ? a.pw : a.ph;
  b.by = TR ? y + a.ph : y * a.sh - a.ph;
  b.bx = TR ? x + pw : x * sw - pw;
  return b;
}

// A k-row as (channel, kz, ky, kx), wave-uniform: decomposed once, then advanced by a constant number of rows per chunk with carries
// (kx against kw, ky against kh, kVol: kz against kd) instead of divisions.  Without a depth axis kz stays 0 and compiles away.
struct KRow { int c, kz, ky, kx; };
struct KStep { int dc, dkz, dky, dkx; };

template <bool VOL>
__device__ __forceinline__ KRow k_row(int kg, int kd, int kh, int kw) {
  const int kk = kh * kw, kkk = VOL ? kd * kk : kk;
  KRow r;
  r.c = kg / kkk;
  int tap = kg - r.c * kkk;
  r.kz = 0;
  if constexpr (VOL) { r.kz = tap / kk; tap -= r.kz * kk; }
  r.ky = tap / kw;
  r.kx = tap - r.ky * kw;
  return r;
}

template <bool VOL>
__device__ __forceinline__ KStep k_step(int rows, int kd, int kh, int kw) {
  const KRow r = k_row<VOL>(rows, kd, kh, kw);
  return KStep{r.c, r.kz, r.ky, r.kx};
}

template <bool VOL>
__device__ __forceinline__ void k_advance(KRow& r, const KStep& d, int kd, int kh, int kw) {
  r.kx += d.dkx;
  if (r.kx >= kw) { r.kx -= kw; ++r.ky; }
  r.ky += d.dky;
  if constexpr (VOL) {
    if (r.ky >= kh) { r.ky -= kh; ++r.kz; }
    r.kz += d.dkz;
    if (r.kz >= kd) { r.kz -= kd; ++r.c; }
  } else {
    if (r.ky >= kh) { r.ky -= kh; ++r.c; }
  }
  r.c += d.dc;
}

// The depth axis of one tap, for all three passes (they all gather through gather_one): the input plane `zi` of the pixel base bz and the
// tap kz, and whether the tap contributes -- forward bz + kz dd inside [0, ID); transposed (bz - kz dd) / sd exact, not negative and below ID.
// An address is formed from `zi` only where this is true.
template <bool TR>
__device__ __forceinline__ bool depth_coord(const GatherDepth& z, int bz, int kz, int& zi) {
  const int oz = kz * z.dd;
  if constexpr (TR) {
    const int tz = bz - oz;
    unsigned qz, rz;
    divmod((unsigned)max(tz, 0), (unsigned)z.sd, z.sd_magic, qz, rz);
    zi = (int)qz;
    return tz >= 0 && rz == 0 && zi < z.ID;
  } else {
    zi = bz + oz;
    return zi >= 0 && zi < z.ID;
  }
}

// col[k-row][pixel] of sample slice `src`; 0 outside the image, beyond K and for a pixel beyond the tile's map
template <bool TR, int GEO>
__device__ __forceinline__ float gather_one(const GatherSrc& a, const GatherDepth& z, const float* src, const KRow& kr, const PixelBase& b) {
  constexpr bool GEN = GEO != kPlain;
  int yi, xi;
  bool ok = b.valid && kr.c < a.C;
  const int oy = GEN ? kr.ky * a.dh : kr.ky, ox = GEN ? kr.kx * a.dw : kr.kx;      // the tap's offset, dilated
  if constexpr (TR) {
    const int ty = b.by - oy, tx = b.bx - ox;
    unsigned qy, ry, qx, rx;
    divmod((unsigned)max(ty, 0), (unsigned)a.sh, a.sh_magic, qy, ry);
    divmod((unsigned)max(tx, 0), (unsigned)(GEN ? a.sw : a.sh), GEN ? a.sw_magic : a.sh_magic, qx, rx);
    yi = (int)qy; xi = (int)qx;
    ok = ok && ty >= 0 && tx >= 0 && ry == 0 && rx == 0 && yi < a.IH && xi < a.IW;
  } else {
    yi = b.by + oy; xi = b.bx + ox;
    ok = ok && yi >= 0 && yi < a.IH && xi >= 0 && xi < a.IW;
  }
  float v = 0.f;
  if constexpr (GEO == kVol) {
    int zi;
    ok = depth_coord<TR>(z, b.bz, kr.kz, zi) && ok;
    if (ok) v = src[((size_t)kr.c * z.ID + zi) * a.IH * a.IW + (size_t)yi * a.IW + xi];
  } else {
    if (ok) v = src[(size_t)kr.c * a.IH * a.IW + (size_t)yi * a.IW + xi];
  }
  return v;
}

// ------------------------------------------------------------------------------------------------ the two gather kernels
struct GatherArgs {
  GatherSrc g;
  const float* wp;          // packed operand
  const float* bias;
  float* out;               // channel c0 of sample 0 of the output blob
  int out_ctot, M, G, ksteps, ptiles, mblocks;
  int relu;
  float slope;
  GatherDepth z;
};

template <bool TR, int NG, int GEO>
__global__ __launch_bounds__(kThreads) void conv_general_gather(GatherArgs a) {
  __shared__ float col[kKC * kColStrideG];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned task = blockIdx.x;
  const int mb = task % a.mblocks; task /= a.mblocks;
  constexpr bool GEN = GEO != kPlain, VOL = GEO == kVol;
  int grp = 0;                // the layer's group: a grid factor; M, G, ksteps and C are those of one group
  if constexpr (GEN) { grp = task % a.g.group; task /= a.g.group; }
  const int pt = task % a.ptiles;
  const int n = task / a.ptiles;
  const long long p0 = (long long)pt * kPix;
  const size_t iplane = (size_t)(VOL ? a.z.ID : 1) * a.g.IH * a.g.IW;
  const float* src = a.g.in + ((size_t)n * a.g.ctot + (size_t)grp * a.g.C) * iplane;
  const PixelBase pb = pixel_base<TR, GEO>(a.g, a.z, p0 + lane);
  const int kd = VOL ? a.z.kd : 1, kh = a.g.kh, kw = GEN ? a.g.kw : a.g.kh;

  // this wave's NG row groups of the weights; beyond the last real one of the group the last one again (computed, not stored)
  const float* wl[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int g = min(NG * mb + j, a.G - 1);
    wl[j] = a.wp + ((size_t)grp * a.G + g) * a.ksteps * 64 + lane;
  }
  f32x4 acc[NG];
#pragma unroll
  for (int j = 0; j < NG; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = a.ksteps / 4;
  const KStep kstep = k_step<VOL>(kKC, kd, kh, kw);
  KRow kr[4];
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    kr[i] = k_row<VOL>(wave + 4 * i, kd, kh, kw);
    v[i] = gather_one<TR, GEO>(a.g, a.z, src, kr[i], pb);
  }
  // the weight operand of a chunk (4 k-steps x NG groups) is fetched a chunk ahead, like the col values
  float w[4][NG];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int j = 0; j < NG; ++j) w[ks][j] = wl[j][(size_t)ks * 64];
  const int arow = (lane >> 4) * kColStrideG + 16 * wave + (lane & 15);
  for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
    for (int i = 0; i < 4; ++i) col[(wave + 4 * i) * kColStrideG + lane] = v[i];
    __syncthreads();
    // the next chunk's loads fly during this chunk's MFMAs (col beyond K: zeros, nothing is loaded; weights: the last chunk again)
    float wn[4][NG];
    const int nx = min(ch + 1, nchunks - 1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < NG; ++j) wn[ks][j] = wl[j][(size_t)(4 * nx + ks) * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k_advance<VOL>(kr[i], kstep, kd, kh, kw);
      v[i] = gather_one<TR, GEO>(a.g, a.z, src, kr[i], pb);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const float av = col[arow + 4 * ks * kColStrideG];
#pragma unroll
      for (int j = 0; j < NG; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[ks][j], acc[j], 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < NG; ++j) w[ks][j] = wn[ks][j];
  }

  // lane (pixel quad lane >> 4, channel lane & 15) holds 4 consecutive pixels of one channel
  const long long p = p0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
  for (int j = 0; j < NG; ++j) {
    const int co = 16 * (NG * mb + j) + (lane & 15);
    if (co >= a.M || p >= a.g.OP) continue;
    const int cg = grp * a.M + co;      // the channel in the layer's slice
    const float bv = a.bias ? a.bias[cg] : 0.f;
    const f32x4 r = mfma::bias_relu4(acc[j], bv, a.relu, a.slope);
    float* o = a.out + ((size_t)n * a.out_ctot + cg) * (size_t)a.g.OP + p;
    if (p + 3 < a.g.OP && (reinterpret_cast<uintptr_t>(o) & 15) == 0) *reinterpret_cast<f32x4*>(o) = r;
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (p + e < a.g.OP) o[e] = r[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgradArgs {
  GatherSrc g;              // the forward gather of the L blob over the S pixel space
  const float* x;           // channel c0 of sample 0 of the S blob
  int x_ctot, A, G, ablocks, ktiles, ptiles;
  long long chunks, per_part, Kpad;
  float* ws;                // [nsplit][group][16 G][Kpad]; A, G, Kpad and g.C are those of one group
  GatherDepth z;
};

// the values of a thread for pixel chunk q: 4 of the col tile (k-rows kr) and 16 of the S blob (channels ch0, ch0 + 4, ... of group grp)
template <int GEO>
__device__ __forceinline__ void wgrad_fetch(const WgradArgs& a, const KRow (&kr)[4], long long q, int grp, int ch0, int lane, float (&cv)[4],
                                            float (&xv)[16]) {
  const int n = (int)(q / a.ptiles);
  const long long p = (q - (long long)n * a.ptiles) * kPix + lane;
  const float* src = a.g.in + ((size_t)n * a.g.ctot + (size_t)grp * a.g.C) * (GEO == kVol ? a.z.ID : 1) * a.g.IH * a.g.IW;
  const PixelBase pb = pixel_base<false, GEO>(a.g, a.z, p);
#pragma unroll
  for (int i = 0; i < 4; ++i) cv[i] = gather_one<false, GEO>(a.g, a.z, src, kr[i], pb);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int ch = ch0 + 4 * i;
    xv[i] = (ch < a.A && pb.valid) ? a.x[((size_t)n * a.x_ctot + (size_t)grp * a.A + ch) * (size_t)a.g.OP + p] : 0.f;
  }
}

template <int GEO>
__global__ __launch_bounds__(kThreads) void conv_general_wgrad(WgradArgs a) {
  constexpr bool GEN = GEO != kPlain, VOL = GEO == kVol;
  __shared__ float col[kKC * kColStrideW];
  __shared__ float xs[64 * kColStrideW];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  unsigned task = blockIdx.x;
  const int kt = task % a.ktiles; task /= a.ktiles;
  const int ab = task % a.ablocks; task /= a.ablocks;
  int grp = 0, ngrp = 1;      // the layer's group: a grid factor, a 64-channel tile stays inside one group
  if constexpr (GEN) { ngrp = a.g.group; grp = task % ngrp; task /= ngrp; }
  const int part = task;
  const long long q0 = (long long)part * a.per_part, q1 = min(q0 + a.per_part, a.chunks);
  const bool active = 4 * ab + wave < a.G;          // a wave beyond the last channel group only helps staging

  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  float cv[4], xv[16];
  KRow kr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) kr[i] = k_row<VOL>(kt * kKC + wave + 4 * i, VOL ? a.z.kd : 1, a.g.kh, GEN ? a.g.kw : a.g.kh);
  // chunk q's values are fetched while chunk q - 1 is multiplied (the last chunk of the part is fetched twice: no branch)
  wgrad_fetch<GEO>(a, kr, q0, grp, 64 * ab + wave, lane, cv, xv);
  for (long long q = q0; q < q1; ++q) {
    __syncthreads();      // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) col[(wave + 4 * i) * kColStrideW + lane] = cv[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) xs[(wave + 4 * i) * kColStrideW + lane] = xv[i];
    __syncthreads();
    wgrad_fetch<GEO>(a, kr, min(q + 1, q1 - 1), grp, 64 * ab + wave, lane, cv, xv);
    if (active) {
      const float* xr = xs + (16 * wave + (lane & 15)) * kColStrideW + (lane >> 4);
      const float* cr = col + (lane & 15) * kColStrideW + (lane >> 4);
#pragma unroll
      for (int st = 0; st < kPix / 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[4 * st], cr[4 * st], acc, 0, 0, 0);
    }
  }
  if (active) {
    // lane holds channels 16 g + 4 (lane >> 4) + r of k-column 16 kt + (lane & 15)
    float* o = a.ws + (((size_t)part * ngrp + grp) * (16 * a.G) + 16 * (4 * ab + wave) + 4 * (lane >> 4)) * (size_t)a.Kpad + (size_t)kt * kKC + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(size_t)r * a.Kpad] = acc[r];
  }
}

// weight_diff[a][k] (+)= the parts in part order; blob row a = (group, row of the group), A rows per group, `rows` = 16 G of them in the workspace
__global__ void conv_general_wgrad_finalize(const float* ws, float* dw, int A, int group, long long K, long long Kpad, int rows, int nsplit, int accumulate) {
  const long long total = (long long)A * group * K, part_rows = (long long)group * rows;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long ch = i / K, k = i - ch * K;
    long long row = ch;
    if (group > 1) {          // (uniform; without groups the workspace rows are the blob's)
      const int grp = (int)ch / A;
      row = (long long)grp * rows + ((int)ch - grp * A);
    }
    float s = ws[row * Kpad + k];
    for (int part = 1; part < nsplit; ++part) s += ws[(part * part_rows + row) * Kpad + k];
    dw[i] = accumulate ? dw[i] + s : s;
  }
}

// bias_diff[c] (+)= sum over (n, pixels) of diff[n][c][.]: thread t adds elements t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(kThreads) void conv_general_bias_grad(const float* diff, int ctot, int N, long long P, float* db, int accumulate) {
  __shared__ float part[kThreads];
  const int c = blockIdx.x;
  const long long total = (long long)N * P;
  float s = 0.f;
  for (long long i = threadIdx.x; i < total; i += kThreads) {
    const long long n = i / P, p = i - n * P;
    s += diff[((size_t)n * ctot + c) * (size_t)P + p];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[c] = accumulate ? db[c] + part[0] : part[0];
}

// ------------------------------------------------------------------------------------------------ packing
// W [Cs][Cl / group][kk] -> Wp[group][g][ks][lane]; swapped: rows are Clg (the transposed gather), else Csg.  The blob rows of group grp are
// [grp Csg, ...): not swapped M = Csg, K = Clg kk; swapped R = Csg, M = Clg
__global__ void conv_general_pack(const float* w, float* wp, int M, int R, int G, int kk, long long K, int ksteps, long long total, int swapped) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const long long r = i >> 6;
    const int ks = (int)(r % ksteps);
    const long long gg = r / ksteps;
    const int grp = (int)(gg / G), g = (int)(gg - (long long)grp * G);
    const int m = 16 * g + (lane & 15);
    const long long kg = 4ll * ks + (lane >> 4);
    float v = 0.f;
    if (m < M && kg < K) {
      const long long c = kg / kk, tap = kg - c * kk;
      v = swapped ? w[(((long long)grp * R + c) * M + m) * kk + tap] : w[((long long)grp * M + m) * K + kg];
    }
    wp[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------ host entry helpers
inline bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

inline void set_taps(GatherSrc& a, GatherDepth& z, const Sides& g) {
  a.kh = g.kh; a.kw = g.kw; a.sh = g.sh; a.sw = g.sw; a.ph = g.ph; a.pw = g.pw; a.dh = g.dh; a.dw = g.dw; a.group = g.group;
  a.sh_magic = div_magic(g.sh); a.sw_magic = div_magic(g.sw);
  z.kd = g.kd; z.sd = g.sd; z.pd = g.pd; z.dd = g.dd; z.sd_magic = div_magic(g.sd);
}

// the input map and the pixel space of a gather: in_l: the input is the larger map (the forward gather), else the smaller one
inline void set_maps(GatherSrc& a, GatherDepth& z, const Sides& g, bool in_l) {
  z.ID = in_l ? g.Dl : g.Ds; a.IH = in_l ? g.Hl : g.Hs; a.IW = in_l ? g.Wl : g.Ws;
  const int OH = in_l ? g.Hs : g.Hl;
  a.OW = in_l ? g.Ws : g.Wl;
  z.OHW = OH * a.OW;        // (below 2^31: a whole blob is)
  a.OP = in_l ? g.Ps() : g.Pl();
  a.ow_magic = div_magic(a.OW); z.ohw_magic = div_magic(z.OHW);
}

int run_gather(const Sides& g, bool tr, const float* in, int in_ctot, int in_c0, const float* packed, const float* bias, float* out, int out_ctot,
               int out_c0, int relu, float slope, hipStream_t st) {
  const Gemm m = pass_gemm(g, tr);
  GatherArgs a;
  set_maps(a.g, a.z, g, !tr);
  set_taps(a.g, a.z, g);
  a.g.in = in + (size_t)in_c0 * (size_t)(tr ? g.Ps() : g.Pl());
  a.g.ctot = in_ctot; a.g.C = m.R;
  a.wp = packed; a.bias = bias;
  a.out = out + (size_t)out_c0 * a.g.OP;
  a.out_ctot = out_ctot; a.M = m.M; a.G = m.G; a.ksteps = m.ksteps;
  const int ng = groups_per_block(m.G);
  a.ptiles = (int)cdivll(a.g.OP, kPix); a.mblocks = (m.G + ng - 1) / ng;
  a.relu = relu; a.slope = slope;
  const long long tiles = gather_tiles(g, tr, m, ng);
  if (tiles > kMaxTiles) return fail(FN2_ERR_UNSUPPORTED, "fn2_conv_general: grid too large");
  const dim3 grid((unsigned)tiles), block(kThreads);
#define FN2_GATHER(TR_, NG_) \
  do { if (g.plain) hipLaunchKernelGGL((conv_general_gather<TR_, NG_, kPlain>), grid, block, 0, st, a); \
       else if (g.volume) hipLaunchKernelGGL((conv_general_gather<TR_, NG_, kVol>), grid, block, 0, st, a); \
       else hipLaunchKernelGGL((conv_general_gather<TR_, NG_, kGen>), grid, block, 0, st, a); } while (0)
  if (tr) { if (ng == 1) FN2_GATHER(true, 1); else if (ng == 2) FN2_GATHER(true, 2); else FN2_GATHER(true, 4); }
  else { if (ng == 1) FN2_GATHER(false, 1); else if (ng == 2) FN2_GATHER(false, 2); else FN2_GATHER(false, 4); }
#undef FN2_GATHER
  return check_launch("fn2_conv_general");
}

int check_slices(const char* what, const Sides& g, int bottom_channels, int bottom_c0, int top_channels, int top_c0) {
  if (bottom_c0 < 0 || bottom_channels < 1 || (long long)bottom_c0 + g.Cin > bottom_channels || top_c0 < 0 || top_channels < 1 ||
      (long long)top_c0 + g.Cout > top_channels)
    return fail(FN2_ERR_INVALID_ARG, "%s: channel slice outside the blob", what);
  return FN2_OK;
}

int refuse(const char* what, const Geom& geom, int transposed) {
  if (geom.null) return fail(FN2_ERR_UNSUPPORTED, "%s: null descriptor", what);
  const int* v = geom.v;
  const char* kind = transposed ? "Deconvolution" : "Convolution";
  if (geom.depth)
    return fail(FN2_ERR_UNSUPPORTED,
                "%s: no kernel for %s N=%d Cin=%d %dx%dx%d Cout=%d kernel=%dx%dx%d stride=%dx%dx%d pad=%dx%dx%d dilation=%dx%dx%d group=%d (invalid, "
                "empty output, or beyond the 32-bit index limits)",
                what, kind, v[kGN], v[kGCin], v[kGDin], v[kGHin], v[kGWin], v[kGCout], v[kGkd], v[kGkh], v[kGkw], v[kGsd], v[kGsh], v[kGsw], v[kGpd],
                v[kGph], v[kGpw], v[kGdd], v[kGdh], v[kGdw], v[kGgroup]);
  return fail(FN2_ERR_UNSUPPORTED,
              "%s: no kernel for %s N=%d Cin=%d %dx%d Cout=%d kernel=%dx%d stride=%dx%d pad=%dx%d dilation=%dx%d group=%d (invalid, empty output, or beyond "
              "the 32-bit index limits)",
              what, kind, v[kGN], v[kGCin], v[kGHin], v[kGWin], v[kGCout], v[kGkh], v[kGkw], v[kGsh], v[kGsw], v[kGph], v[kGpw], v[kGdh], v[kGdw],
              v[kGgroup]);
}

// ------------------------------------------------------------------------------------------------ the entry points, on the 19 ints
int geom_sizes(const char* what, const Geom& geom, int transposed, size_t* forward_packed, size_t* backward_data_packed, size_t* backward_weights_packed,
               size_t* backward_weights_workspace) {
  if (forward_packed) *forward_packed = 0;
  if (backward_data_packed) *backward_data_packed = 0;
  if (backward_weights_packed) *backward_weights_packed = 0;
  if (backward_weights_workspace) *backward_weights_workspace = 0;
  Sides g;
  if (!supported(geom, transposed, g)) return refuse(what, geom, transposed);
  if (forward_packed) *forward_packed = packed_floats(g, pass_gemm(g, pass_is_tr(transposed, 0)));
  if (backward_data_packed) *backward_data_packed = packed_floats(g, pass_gemm(g, pass_is_tr(transposed, 1)));
  if (backward_weights_workspace) *backward_weights_workspace = make_wgrad(g).workspace_bytes;
  return FN2_OK;
}

int geom_pack_weights(const char* what, const Geom& geom, int transposed, int pass, const float* weight, float* packed, void* stream) {
  Sides g;
  if (!supported(geom, transposed, g)) return refuse(what, geom, transposed);
  if (pass < 0 || pass > 2) return fail(FN2_ERR_INVALID_ARG, "%s: pass %d (0 forward, 1 data gradient, 2 weight gradient)", what, pass);
  if (pass == 2) return FN2_OK;      // the weight gradient has no weight operand
  if (!weight || !packed) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (misaligned(weight) || misaligned(packed)) return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  const bool tr = pass_is_tr(transposed, pass);
  const Gemm m = pass_gemm(g, tr);
  const long long total = (long long)packed_floats(g, m);
  hipLaunchKernelGGL(conv_general_pack, dim3(blocks_for(total, 256)), dim3(256), 0, as_stream(stream), weight, packed, m.M, m.R, m.G, g.taps(), m.K,
                     m.ksteps, total, tr ? 1 : 0);
  return check_launch(what);
}

int geom_forward(const char* what, const Geom& geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0, const float* packed_weight,
                 const float* bias, float* top, int top_channels, int top_c0, int relu, float negative_slope, void* stream) {
  Sides g;
  if (!supported(geom, transposed, g)) return refuse(what, geom, transposed);
  if (!bottom || !packed_weight || !top) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, g, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(bottom) || misaligned(packed_weight) || misaligned(top) || misaligned(bias))
    return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  return run_gather(g, pass_is_tr(transposed, 0), bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels, top_c0, relu,
                    negative_slope, as_stream(stream));
}

int geom_backward_data(const char* what, const Geom& geom, int transposed, const float* top_diff, int top_channels, int top_c0,
                       const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream) {
  Sides g;
  if (!supported(geom, transposed, g)) return refuse(what, geom, transposed);
  if (!top_diff || !packed_weight || !bottom_diff) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, g, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(top_diff) || misaligned(packed_weight) || misaligned(bottom_diff)) return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  return run_gather(g, pass_is_tr(transposed, 1), top_diff, top_channels, top_c0, packed_weight, nullptr, bottom_diff, bottom_channels, bottom_c0, 0,
                    0.f, as_stream(stream));
}

int geom_backward_weights(const char* what, const Geom& geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                          const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff, int accumulate, void* workspace,
                          size_t workspace_bytes, void* stream) {
  Sides g;
  if (!supported(geom, transposed, g)) return refuse(what, geom, transposed);
  if (!bottom || !top_diff || !weight_diff) return fail(FN2_ERR_INVALID_ARG, "%s: null blob", what);
  if (const int rc = check_slices(what, g, bottom_channels, bottom_c0, top_channels, top_c0)) return rc;
  if (misaligned(bottom) || misaligned(top_diff) || misaligned(weight_diff) || misaligned(bias_diff) || misaligned(workspace))
    return fail(FN2_ERR_INVALID_ARG, "%s: blobs must be 4-byte aligned", what);
  const WgradPlan p = make_wgrad(g);
  if (!workspace || workspace_bytes < p.workspace_bytes)
    return fail(FN2_ERR_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", what, p.workspace_bytes, workspace ? workspace_bytes : (size_t)0);
  hipStream_t st = as_stream(stream);
  // the S blob multiplies the forward gather of the L blob
  const float* sblob = transposed ? bottom : top_diff;
  const int s_ctot = transposed ? bottom_channels : top_channels, s_c0 = transposed ? bottom_c0 : top_c0;
  const float* lblob = transposed ? top_diff : bottom;
  const int l_ctot = transposed ? top_channels : bottom_channels, l_c0 = transposed ? top_c0 : bottom_c0;
  WgradArgs a;
  set_maps(a.g, a.z, g, true);
  set_taps(a.g, a.z, g);
  a.g.in = lblob + (size_t)l_c0 * (size_t)g.Pl();
  a.g.ctot = l_ctot; a.g.C = p.m.R;
  a.x = sblob + (size_t)s_c0 * a.g.OP;
  a.x_ctot = s_ctot; a.A = p.m.M; a.G = p.m.G; a.ablocks = (p.m.G + 3) / 4; a.ktiles = (int)(p.m.Kpad / kKC); a.ptiles = p.ptiles;
  a.chunks = p.chunks; a.per_part = p.per_part; a.Kpad = p.m.Kpad;
  a.ws = static_cast<float*>(workspace);
  if (g.plain) hipLaunchKernelGGL(conv_general_wgrad<kPlain>, dim3((unsigned)p.tiles), dim3(kThreads), 0, st, a);
  else if (g.volume) hipLaunchKernelGGL(conv_general_wgrad<kVol>, dim3((unsigned)p.tiles), dim3(kThreads), 0, st, a);
  else hipLaunchKernelGGL(conv_general_wgrad<kGen>, dim3((unsigned)p.tiles), dim3(kThreads), 0, st, a);
  if (const int rc = check_launch(what)) return rc;
  hipLaunchKernelGGL(conv_general_wgrad_finalize, dim3(blocks_for((long long)g.Cs * p.m.K, 256)), dim3(256), 0, st, a.ws, weight_diff, p.m.M, g.group,
                     p.m.K, p.m.Kpad, 16 * p.m.G, p.nsplit, accumulate);
  if (const int rc = check_launch(what)) return rc;
  if (bias_diff) {
    const long long Pt = transposed ? g.Pl() : g.Ps();
    hipLaunchKernelGGL(conv_general_bias_grad, dim3((unsigned)g.Cout), dim3(kThreads), 0, st, top_diff + (size_t)top_c0 * Pt, top_channels, g.N, Pt,
                       bias_diff, accumulate);
    if (const int rc = check_launch(what)) return rc;
  }
  return FN2_OK;
}

}  // namespace
}  // namespace fn2

using namespace fn2;

FN2_API int fn2_conv_general_supported(const fn2_conv_desc* desc, int transposed) {
  Sides g;
  return supported(Geom::from_desc(desc), transposed, g) ? 1 : 0;
}

FN2_API int fn2_debug_set_conv_general_groups(int groups) {
  if (groups != 0 && groups != 1 && groups != 2 && groups != 4)
    return fail(FN2_ERR_INVALID_ARG, "fn2_debug_set_conv_general_groups: %d (0 = by geometry, 1, 2 or 4)", groups);
  forced_groups() = groups;
  return FN2_OK;
}

// the square-tap entry points (include/flownet2_hip_conv_general.h): the same code with (k, k, s, s, p, p, 1, 1, 1)
FN2_API int fn2_conv_general_sizes(const fn2_conv_desc* desc, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                                   size_t* backward_weights_packed, size_t* backward_weights_workspace) {
  const Geom d = Geom::from_desc(desc);
  return geom_sizes("fn2_conv_general_sizes", d, transposed, forward_packed, backward_data_packed, backward_weights_packed,
                    backward_weights_workspace);
}

FN2_API int fn2_conv_general_pack_weights(const fn2_conv_desc* desc, int transposed, int pass, const float* weight, float* packed, void* stream) {
  const Geom d = Geom::from_desc(desc);
  return geom_pack_weights("fn2_conv_general_pack_weights", d, transposed, pass, weight, packed, stream);
}

FN2_API int fn2_conv_general_forward(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                     const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                                     int relu, float negative_slope, void* stream) {
  const Geom d = Geom::from_desc(desc);
  return geom_forward("fn2_conv_general_forward", d, transposed, bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels,
                      top_c0, relu, negative_slope, stream);
}

FN2_API int fn2_conv_general_backward_data(const fn2_conv_desc* desc, int transposed, const float* top_diff, int top_channels, int top_c0,
                                           const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream) {
  const Geom d = Geom::from_desc(desc);
  return geom_backward_data("fn2_conv_general_backward_data", d, transposed, top_diff, top_channels, top_c0, packed_weight, bottom_diff,
                            bottom_channels, bottom_c0, stream);
}

FN2_API int fn2_conv_general_backward_weights(const fn2_conv_desc* desc, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                              const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                              int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  const Geom d = Geom::from_desc(desc);
  return geom_backward_weights("fn2_conv_general_backward_weights", d, transposed, bottom, bottom_channels, bottom_c0, top_diff, top_channels,
                               top_c0, weight_diff, bias_diff, accumulate, workspace, workspace_bytes, stream);
}

// the 14-int entry points (include/flownet2_hip_conv_geometry.h)
FN2_API int fn2_conv_geometry_supported(const int* geom, int transposed) {
  Sides g;
  return supported(Geom::from_planar(geom), transposed, g) ? 1 : 0;
}

FN2_API int fn2_conv_geometry_out_shape(const int* geom, int transposed, int* out_h, int* out_w) {
  if (out_h) *out_h = 0;
  if (out_w) *out_w = 0;
  Sides g;
  const Geom d = Geom::from_planar(geom);
  if (!supported(d, transposed, g)) return refuse("fn2_conv_geometry_out_shape", d, transposed);
  if (out_h) *out_h = transposed ? g.Hl : g.Hs;
  if (out_w) *out_w = transposed ? g.Wl : g.Ws;
  return FN2_OK;
}

FN2_API int fn2_conv_geometry_sizes(const int* geom, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                                    size_t* backward_weights_packed, size_t* backward_weights_workspace) {
  return geom_sizes("fn2_conv_geometry_sizes", Geom::from_planar(geom), transposed, forward_packed, backward_data_packed, backward_weights_packed,
                    backward_weights_workspace);
}

FN2_API int fn2_conv_geometry_pack_weights(const int* geom, int transposed, int pass, const float* weight, float* packed, void* stream) {
  return geom_pack_weights("fn2_conv_geometry_pack_weights", Geom::from_planar(geom), transposed, pass, weight, packed, stream);
}

FN2_API int fn2_conv_geometry_forward(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                      const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                                      int relu, float negative_slope, void* stream) {
  return geom_forward("fn2_conv_geometry_forward", Geom::from_planar(geom), transposed, bottom, bottom_channels, bottom_c0, packed_weight, bias, top, top_channels, top_c0,
                      relu, negative_slope, stream);
}

FN2_API int fn2_conv_geometry_backward_data(const int* geom, int transposed, const float* top_diff, int top_channels, int top_c0,
                                            const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream) {
  return geom_backward_data("fn2_conv_geometry_backward_data", Geom::from_planar(geom), transposed, top_diff, top_channels, top_c0, packed_weight, bottom_diff,
                            bottom_channels, bottom_c0, stream);
}

FN2_API int fn2_conv_geometry_backward_weights(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                               const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                               int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  return geom_backward_weights("fn2_conv_geometry_backward_weights", Geom::from_planar(geom), transposed, bottom, bottom_channels, bottom_c0, top_diff, top_channels,
                               top_c0, weight_diff, bias_diff, accumulate, workspace, workspace_bytes, stream);
}

// the 19-int entry points (include/flownet2_hip_conv_volume.h)
FN2_API int fn2_conv_volume_supported(const int* geom, int transposed) {
  Sides g;
  return supported(Geom::from_volume(geom), transposed, g) ? 1 : 0;
}

FN2_API int fn2_conv_volume_out_shape(const int* geom, int transposed, int* out_d, int* out_h, int* out_w) {
  if (out_d) *out_d = 0;
  if (out_h) *out_h = 0;
  if (out_w) *out_w = 0;
  Sides g;
  const Geom d = Geom::from_volume(geom);
  if (!supported(d, transposed, g)) return refuse("fn2_conv_volume_out_shape", d, transposed);
  if (out_d) *out_d = transposed ? g.Dl : g.Ds;
  if (out_h) *out_h = transposed ? g.Hl : g.Hs;
  if (out_w) *out_w = transposed ? g.Wl : g.Ws;
  return FN2_OK;
}

FN2_API int fn2_conv_volume_sizes(const int* geom, int transposed, size_t* forward_packed, size_t* backward_data_packed,
                                  size_t* backward_weights_packed, size_t* backward_weights_workspace) {
  return geom_sizes("fn2_conv_volume_sizes", Geom::from_volume(geom), transposed, forward_packed, backward_data_packed, backward_weights_packed,
                    backward_weights_workspace);
}

FN2_API int fn2_conv_volume_pack_weights(const int* geom, int transposed, int pass, const float* weight, float* packed, void* stream) {
  return geom_pack_weights("fn2_conv_volume_pack_weights", Geom::from_volume(geom), transposed, pass, weight, packed, stream);
}

FN2_API int fn2_conv_volume_forward(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                    const float* packed_weight, const float* bias, float* top, int top_channels, int top_c0,
                                    int relu, float negative_slope, void* stream) {
  return geom_forward("fn2_conv_volume_forward", Geom::from_volume(geom), transposed, bottom, bottom_channels, bottom_c0, packed_weight, bias, top,
                      top_channels, top_c0, relu, negative_slope, stream);
}

FN2_API int fn2_conv_volume_backward_data(const int* geom, int transposed, const float* top_diff, int top_channels, int top_c0,
                                          const float* packed_weight, float* bottom_diff, int bottom_channels, int bottom_c0, void* stream) {
  return geom_backward_data("fn2_conv_volume_backward_data", Geom::from_volume(geom), transposed, top_diff, top_channels, top_c0, packed_weight,
                            bottom_diff, bottom_channels, bottom_c0, stream);
}

FN2_API int fn2_conv_volume_backward_weights(const int* geom, int transposed, const float* bottom, int bottom_channels, int bottom_c0,
                                             const float* top_diff, int top_channels, int top_c0, float* weight_diff, float* bias_diff,
                                             int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  return geom_backward_weights("fn2_conv_volume_backward_weights", Geom::from_volume(geom), transposed, bottom, bottom_channels, bottom_c0, top_diff,
                               top_channels, top_c0, weight_diff, bias_diff, accumulate, workspace, workspace_bytes, stream);
}
