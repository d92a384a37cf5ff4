// orbx_plan.hip — the extractor's host plan (orbx_plan.h).
//
// The constructor arithmetic of ORBextractor (src/ORBextractor.cc:496-560)
// and the per-level geometry of ComputePyramid / ComputeKeyPointsOctTree /
// DistributeOctTree are evaluated once per (config, frame size) on the host
// in the same float arithmetic as the reference, and shipped to the kernels
// as tables: resize coefficients, the FAST cell list with its slot ranges,
// quadtree roots. Nothing here calls the HIP runtime: a plan can be built and
// checked on a machine with no device.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_hostutil.h"
#include "orbx_plan.h"

using namespace orbx;

static inline int cv_round(float v) { return (int)lrintf(v); }
static inline int cv_floor(float v) { int i = (int)v; return i - (i > v); }
static inline short sat_short(int v) { return (short)std::min(std::max(v, (int)SHRT_MIN), (int)SHRT_MAX); }

// m = ceil(2^32 / d): mulhi(id, m) equals id / d while id * (m * d - 2^32) < 2^32 (ids < d * batch)
unsigned orbx::exact_div_magic(unsigned long long d, unsigned long long batch) {
  if (d <= 1) return 0u;
  const unsigned long long m = ((1ull << 32) + d - 1) / d, e = m * d - (1ull << 32);
  return d * batch * e < (1ull << 32) ? (unsigned)m : 0u;
}

// ORBextractor::ORBextractor scalar tables (src/ORBextractor.cc:500-532) and
// umax (:540-555); the fork's scale override (:674-680) in mode F.
void orbx::compute_scales(const orbx_config& c, ScaleTables& t) {
  const int L = c.nlevels;
  t.scale.assign(L, 1.f);
  t.sigma2.assign(L, 1.f);
  for (int i = 1; i < L; i++) {
    t.scale[i] = t.scale[i - 1] * c.scale_factor;
    t.sigma2[i] = t.scale[i] * t.scale[i];
  }
  t.inv_scale.resize(L);
  t.inv_sigma2.resize(L);
  for (int i = 0; i < L; i++) {
    t.inv_scale[i] = 1.0f / t.scale[i];
    t.inv_sigma2[i] = 1.0f / t.sigma2[i];
  }
  t.nfeat.assign(L, 0);
  const float factor = 1.0f / c.scale_factor;
  float nDesired = c.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
  int sum = 0;
  for (int l = 0; l < L - 1; l++) {
    t.nfeat[l] = cv_round(nDesired);
    sum += t.nfeat[l];
    nDesired *= factor;
  }
  t.nfeat[L - 1] = std::max(c.nfeatures - sum, 0);
  const int HP = kHalfPatch;
  int v, v0;
  const int vmax = cv_floor(HP * sqrtf(2.f) / 2 + 1);
  const int vmin = (int)std::ceil(HP * sqrtf(2.f) / 2);
  const double hp2 = HP * HP;
  for (v = 0; v <= vmax; ++v) t.umax[v] = (int)lrint(sqrt(hp2 - v * v));
  for (v = HP, v0 = 0; v >= vmin; --v) {
    while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
    t.umax[v] = v0;
    ++v0;
  }
  if (c.scale_mode == ORBX_SCALE_F) {
    for (int l = 0; l < L; ++l) {
      const unsigned vw = (unsigned)std::ceil(c.width * std::pow(0.8408964, l));
      t.scale[l] = ((float)c.width) / vw;
      t.inv_scale[l] = ((float)vw) / c.width;
    }
  }
}

// getGaussianKernel(7, 2, CV_32F) -> CV_32S x256 (the 8U smooth branch of
// createSeparableLinearFilter): [18, 34, 49, 55, 49, 34, 18].
static void gaussian7(int k[7]) {
  float cf[7];
  double sum = 0;
  for (int i = 0; i < 7; ++i) {
    const double x = i - 3.0;
    cf[i] = (float)std::exp(-0.5 / (2.0 * 2.0) * x * x);
    sum += cf[i];
  }
  sum = 1. / sum;
  for (int i = 0; i < 7; ++i) cf[i] = (float)(cf[i] * sum);
  for (int i = 0; i < 7; ++i) k[i] = cv_round(cf[i] * 256.f);
}

// OpenCV 3.x INTER_LINEAR coefficient tables from (sw,sh) to (dw,dh):
// x entries {sx, a0 | a1<<16}, y entries {sy0 | sy1<<16, b0 | b1<<16}.
static void resize_tables(int sw, int sh, int dw, int dh, std::vector<int2>& xt, std::vector<int2>& yt,
                          int* xmax_out, int* area2x) {
  const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
  const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
  const int isx = (int)lrint(scale_x), isy = (int)lrint(scale_y);
  const bool fast = std::fabs(scale_x - isx) < DBL_EPSILON && std::fabs(scale_y - isy) < DBL_EPSILON;
  *area2x = (fast && isx == 2 && isy == 2) ? 1 : 0;
  xt.resize(dw);
  yt.resize(dh);
  int xmax = dw;
  for (int dx = 0; dx < dw; ++dx) {
    float fx = (float)((dx + 0.5) * scale_x - 0.5);
    int sx = cv_floor(fx);
    fx -= sx;
    if (sx < 0) { fx = 0; sx = 0; }
    if (sx + 1 >= sw) {
      xmax = std::min(xmax, dx);
      if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
    }
    const int a0 = sat_short(cv_round((1.f - fx) * 2048)), a1 = sat_short(cv_round(fx * 2048));
    xt[dx] = make_int2(sx, (a0 & 0xFFFF) | (a1 << 16));
  }
  *xmax_out = xmax;
  auto clip = [](int x, int a, int b) { return x >= a ? (x < b ? x : b - 1) : a; };
  for (int dy = 0; dy < dh; ++dy) {
    float fy = (float)((dy + 0.5) * scale_y - 0.5);
    int sy = cv_floor(fy);
    fy -= sy;
    const int b0 = sat_short(cv_round((1.f - fy) * 2048)), b1 = sat_short(cv_round(fy * 2048));
    yt[dy] = make_int2(clip(sy, 0, sh) | (clip(sy + 1, 0, sh) << 16), (b0 & 0xFFFF) | (b1 << 16));
  }
}

// Row bands of the one-launch pyramid (orbx_pyramid.hip pyr_band_kernel).
// Bands of R rows partition the last level; walking down, a band's rows at
// level l start at the first source row of its first row at level l+1, and it
// OWNS (writes) the rows up to where the next band's start; it COMPUTES its
// own rows plus every source row its level-(l+1) rows read. Level 0 rows are
// only read. R shrinks until the two LDS row buffers fit; if even R = 1 does
// not, the per-level kernel is used.
// Column tiles split every band the same way (rows and columns are
// separable): tile c of the last level owns an even-aligned share of its
// columns; walking down, its columns at level l start at the first source
// column of its first column at level l+1 (rounded down to even, so that the
// owned ranges of every level start even and a 2-column store never straddles
// two tiles), and it computes every source column its level-(l+1) columns read.
// Per (tile, level) the table holds {comp_lo, comp_hi}, {own_lo, own_hi} and
// {LDS row pitch, LDS origin}: the column of LDS byte 0 (level 0, staged in
// 16-byte chunks: comp_lo rounded down to 16; else comp_lo).
struct PyrCols {
  int nct = 1;
  std::vector<int> lo, chi, ohi;  // [tile][level]
  int lpitch[kMaxLevels] = {};    // LDS row pitch per level (the widest tile)
};

static bool plan_pyr_cols(const ExtractParams& P, const std::vector<int2>& rtab, int nct, PyrCols& C) {
  const int L = P.L, WL = P.lv[L - 1].w;
  if (nct > 1 && WL / nct < 32) return false;  // tiles of >= 32 last-level columns
  C.nct = nct;
  C.lo.assign((size_t)nct * L, 0);
  C.chi.assign((size_t)nct * L, 0);
  C.ohi.assign((size_t)nct * L, 0);
  // source columns of output column x at level l (>= 1): sx and sx + 1 (xtab2
  // folds the 2x area case in as {2x, 0}); past the last column, the last one's
  auto src_lo_x = [&](int l, int x) { return rtab[P.lv[l].xtab2 + std::min(x, P.lv[l].w - 1)].x; };
  auto src_hi_x = [&](int l, int x) { return rtab[P.lv[l].xtab2 + std::min(x, P.lv[l].w - 1)].x + 1; };
  for (int c = 0; c < nct; ++c) {
    C.lo[c * L + L - 1] = c == 0 ? 0 : ((int)((long long)c * WL / nct) & ~1);
    C.chi[c * L + L - 1] = C.ohi[c * L + L - 1] = (c + 1 < nct ? ((int)((long long)(c + 1) * WL / nct) & ~1) : WL) - 1;
  }
  for (int l = L - 2; l >= 0; --l)
    for (int c = 0; c < nct; ++c) C.lo[c * L + l] = c == 0 ? 0 : (src_lo_x(l + 1, C.lo[c * L + l + 1]) & ~1);
  for (int l = L - 2; l >= 0; --l)
    for (int c = 0; c < nct; ++c) {
      const int own_hi = c + 1 < nct ? C.lo[(c + 1) * L + l] - 1 : P.lv[l].w - 1;
      if (own_hi < C.lo[c * L + l]) return false;  // a tile with no column of its own
      C.ohi[c * L + l] = own_hi;
      C.chi[c * L + l] = std::max(src_hi_x(l + 1, C.chi[c * L + l + 1]), l > 0 ? own_hi : 0);
    }
  for (int l = 0; l < L; ++l) {
    int p = 0;
    for (int c = 0; c < nct; ++c) {
      const int lo = C.lo[c * L + l], hi = C.chi[c * L + l];
      // level 0: 16-byte chunks from lo & ~15 up to column hi (the last sx + 1
      // read; past the image it reads an unstaged byte, weighted 0); other
      // levels: the 2-column runs of G = ceil(width / 8) groups end <= 6 past hi
      p = std::max(p, l == 0 ? ((hi - (lo & ~15) + 1 + 15) & ~15) : ((hi - lo + 1 + 8 + 15) & ~15));
    }
    // experiments: ORBX_PYR_PADMOD=m pads every LDS row pitch to m mod 128
    // (level 0 keeps its 16-byte rows: m rounded down to 16 there)
    if (const char* e = getenv("ORBX_PYR_PADMOD")) {
      const int m = (l == 0 ? atoi(e) & ~15 : atoi(e)) % 128, step = l == 0 ? 16 : 4;
      while (p % 128 != m) p += step;
    }
    C.lpitch[l] = p;
  }
  // pyr_band_kernel maps its 512 threads to G = ceil(width / 8) column groups
  // x 512 / G row chunks, and reads aligned dwords from its LDS rows (true
  // today: level sides are at most 4096 and pitches are rounded to 16)
  for (int l = 1; l < L; ++l) {
    if (C.lpitch[l - 1] % 4) return false;
    for (int c = 0; c < nct; ++c)
      if (C.chi[c * L + l] - C.lo[c * L + l] + 1 > 8 * 512) return false;
  }
  return true;
}

// The bounds of plan q's column records (written by plan_band_pyramid, read by
// pyr_band_kernel) as code: every record lies inside the table at a 16-byte
// boundary; a run's dword pair starts at a multiple of 4 inside the source
// level's LDS row or at most 8 bytes past its pitch (a thread's runs end up to
// 6 columns past the tile's computed ones, at most 12 source columns at scale
// 2, and a row pitch holds 9 spare bytes, level 0's 1), so that its 8 bytes end
// at most 16 past the row: in the next row, or in the 16 spare bytes that end
// the kernel's LDS block; a selector picks
// bytes 0..7 of the pair; and a run flagged for a store lies inside the tile's
// owned columns, which lie inside the level; and the bands' row entries (below).
// plan_band_pyramid refuses a plan
// that fails (the per-level kernel runs instead). Returns the records checked,
// or -1.
static long long pyr_records_ok(const ExtractParams& P, const std::vector<int2>& rtab,
                                const ExtractParams::PyrPlan& q) {
  const int L = P.L;
  long long n = 0;
  // a band's staged row entries: inside the table, one per computed row of
  // levels 1 .. L-1, within the LDS bytes the plan sets aside for them
  for (int b = 0; b < q.nbands; ++b) {
    const int2* bt = rtab.data() + q.bands + (long long)b * L * 2;
    long long rows = 0;
    for (int l = 1; l < L; ++l) rows += bt[2 * l].y - bt[2 * l].x + 1;
    const int2 yh = bt[1];
    if (yh.x <= 0 || yh.y != rows || (long long)yh.x + yh.y > (long long)rtab.size() || rows * 8 > q.lds_y) return -1;
  }
  for (int t = 0; t < q.nct; ++t)
    for (int l = 1; l < L; ++l) {
      const int2* xt = rtab.data() + q.ctiles + ((long long)t * L + l) * 4;
      const int2 xc = xt[0], xo = xt[1], sp = xt[-4 + 2];
      const int G = (xc.y - xc.x + 1 + 7) >> 3;
      const long long at = xt[3].x;
      if (at <= 0 || (at & 1) || at + 12LL * G > (long long)rtab.size()) return -1;
      if (xo.x < 0 || xo.y >= P.lv[l].w || xo.x > xo.y) return -1;
      for (int gi = 0; gi < G; ++gi, ++n) {
        const uint32_t* rec = (const uint32_t*)(rtab.data() + at + 12LL * gi);
        for (int k = 0; k < 4; ++k) {
          const int off = (int)rec[k], gx = xc.x + 2 * (gi + k * G);
          if (off < 0 || (off & 3) || off > sp.x + 8) return -1;
          for (int j = 0; j < 2; ++j) {
            const uint32_t sel = rec[4 + 2 * k + j], o = sel & 0xFF;
            if (sel != (0x0c000c00u | o | ((o + 1) << 16)) || o > 6) return -1;
          }
          if (((rec[20] >> k) & 1) && (gx < xo.x || gx + 1 > xo.y)) return -1;
          if (((rec[20] >> (4 + k)) & 1) && gx != xo.y) return -1;
        }
        if (rec[20] >> 8) return -1;
      }
    }
  return n;
}

static void plan_band_pyramid(ExtractParams& P, std::vector<int2>& rtab) {
  P.pyr_fused = 0;
  const int L = P.L;
  if (L < 2) return;
  auto src_lo = [&](int l, int y) { return P.lv[l].area2x ? 2 * y : (rtab[P.lv[l].ytab + y].x & 0xFFFF); };
  auto src_hi = [&](int l, int y) { return P.lv[l].area2x ? 2 * y + 1 : (rtab[P.lv[l].ytab + y].x >> 16); };
  const int HL = P.lv[L - 1].h;
  // Candidate tilings: band heights R from a quarter of the last level down
  // to R0/3 (R0 = HL/18) x 1, 2 or 4 column tiles, within a CU's LDS (two
  // workgroups per CU up to budgets[0]). launch_pyramid picks one per launch
  // (pick_pyr_plan); up to 8 are kept (below).
  const size_t budgets[2] = {78 * 1024, 160 * 1024 - 1024};
  const int R0 = std::max(1, (HL + 17) / 18);
  struct Cand {
    int R, nb, nct;
    size_t need0, need1, ybytes;
    long long cost;
    std::vector<int> lo, chi, ohi;
    PyrCols cols;
  };
  std::vector<Cand> cands;
  PyrCols colplans[3];
  bool colok[3];
  for (int k = 0; k < 3; ++k) colok[k] = plan_pyr_cols(P, rtab, 1 << k, colplans[k]);
  // band heights from a quarter of the last level (4 bands: one workgroup
  // per CU for a 32-64-frame batch once tiled) down to R0 / 3
  const int Rmax = std::max(R0 + 5, (HL + 3) / 4);
  for (int R = Rmax; R >= std::max(1, R0 / 3); --R) {
    const int nb = (HL + R - 1) / R;
    if (!cands.empty() && cands.back().nb == nb) continue;  // same band count as a taller R
    std::vector<int> lo((size_t)nb * L), chi((size_t)nb * L), ohi((size_t)nb * L);
    for (int b = 0; b < nb; ++b) {
      lo[b * L + L - 1] = b * R;
      chi[b * L + L - 1] = ohi[b * L + L - 1] = std::min((b + 1) * R, HL) - 1;
    }
    for (int l = L - 2; l >= 0; --l)
      for (int b = 0; b < nb; ++b) lo[b * L + l] = b == 0 ? 0 : src_lo(l + 1, lo[b * L + l + 1]);
    for (int l = L - 2; l >= 0; --l)
      for (int b = 0; b < nb; ++b) {
        const int own_hi = b + 1 < nb ? lo[(b + 1) * L + l] - 1 : P.lv[l].h - 1;
        ohi[b * L + l] = own_hi;
        chi[b * L + l] = std::max(src_hi(l + 1, chi[b * L + l + 1]), l > 0 ? own_hi : 0);
      }
    size_t ybytes = 0;
    for (int b = 0; b < nb; ++b) {
      size_t s = 0;
      for (int l = 1; l < L; ++l) s += (size_t)(chi[b * L + l] - lo[b * L + l] + 1) * 8;
      ybytes = std::max(ybytes, s);
    }
    for (int k = 0; k < 3; ++k) {
      if (!colok[k]) continue;
      const PyrCols& C = colplans[k];
      size_t need[2] = {0, 0};
      for (int l = 0; l < L; ++l) {
        int rows = 0;
        for (int b = 0; b < nb; ++b) rows = std::max(rows, chi[b * L + l] - lo[b * L + l] + 1);
        need[l & 1] = std::max(need[l & 1], (size_t)rows * C.lpitch[l]);
      }
      need[0] = (need[0] + 15) & ~(size_t)15;
      need[1] = (need[1] + 15) & ~(size_t)15;
      if (need[0] + need[1] + ybytes + 16 > budgets[1]) continue;  // a CU's LDS (occupancy 1 above budgets[0])
      long long cost = 0;
      for (int b = 0; b < nb; ++b)
        for (int c = 0; c < C.nct; ++c) {
          long long s = 0;
          for (int l = 0; l < L; ++l)
            s += (long long)(chi[b * L + l] - lo[b * L + l] + 1) * (C.chi[c * L + l] - C.lo[c * L + l] + 1);
          cost = std::max(cost, s);
        }
      cands.push_back(Cand{R, nb, C.nct, need[0], need[1], ybytes, cost, lo, chi, ohi, C});
    }
  }
  if (cands.empty()) return;
  // the plans kept: the one-tile plans (band heights as before column tiles
  // existed; the default first: R0's or the nearest), then for small batches
  // the column-tiled plan that pick_pyr_plan would take in one round
  std::vector<int> keep;
  // experiments (tools/pyr_plans.py): ORBX_PYR_KEEP="nb:nct,nb:nct,..." keeps
  // exactly those candidates (up to 8, in that order)
  const char* ek = getenv("ORBX_PYR_KEEP");
  if (ek) {
    for (const char* p = ek; *p && keep.size() < 8;) {
      int nb = 0, nct = 0, used = 0;
      if (sscanf(p, "%d:%d%n", &nb, &nct, &used) != 2) break;
      for (int i = 0; i < (int)cands.size(); ++i)
        if (cands[i].nb == nb && cands[i].nct == nct) keep.push_back(i);
      p += used;
      if (*p == ',') ++p;
    }
  }
  if (keep.empty()) {
    // the default (R0's band height or the nearest, one tile), then what the
    // launch-time rule (pick_pyr_plan) takes for batches of 1 .. 64 and B on
    // a 256-CU chip (two workgroups per CU up to 78 KB of LDS, else one: the
    // occupancy API sets the real count afterwards), then one-tile plans near R0
    int def = -1;
    for (int i = 0; i < (int)cands.size(); ++i)
      if (cands[i].nct == 1 && cands[i].need0 + cands[i].need1 + cands[i].ybytes + 16 <= budgets[0] &&
          (def < 0 || std::abs(cands[i].nb - (HL + R0 - 1) / R0) < std::abs(cands[def].nb - (HL + R0 - 1) / R0)))
        def = i;
    if (def < 0) def = 0;
    keep.push_back(def);
    std::vector<ExtractParams::PyrPlan> sim(cands.size());
    for (size_t i = 0; i < cands.size(); ++i) {
      sim[i].nbands = cands[i].nb;
      sim[i].nct = cands[i].nct;
      sim[i].cost = (int)cands[i].cost;
      sim[i].occ = cands[i].need0 + cands[i].need1 + cands[i].ybytes + 16 <= budgets[0] ? 2 : 1;
    }
    const int batches[8] = {1, 2, 4, 8, 16, 32, 64, P.B};
    for (int bt : batches) {
      const int best = pick_pyr_plan(sim.data(), (int)sim.size(), bt, 256);
      if (keep.size() < 8 && std::find(keep.begin(), keep.end(), best) == keep.end()) keep.push_back(best);
    }
    for (int d = 1; keep.size() < 8 && d < (int)cands.size(); ++d)
      for (int i : {def - d, def + d})
        if (i >= 0 && i < (int)cands.size() && cands[i].nct == 1 && keep.size() < 8 &&
            std::find(keep.begin(), keep.end(), i) == keep.end())
          keep.push_back(i);
  }
  P.pyr_nplans = 0;
  for (int i : keep) {
    const Cand& c = cands[i];
    ExtractParams::PyrPlan& q = P.pyr_plan[P.pyr_nplans++];
    q.nbands = c.nb;
    q.nct = c.nct;
    q.lds_a = (int)c.need0;
    q.lds_b = (int)c.need1;
    q.lds_y = (int)c.ybytes;
    q.cost = (int)c.cost;
    q.occ = 0;
    q.bands = (int)rtab.size();
    for (int b = 0; b < c.nb; ++b)
      for (int l = 0; l < L; ++l) {
        rtab.push_back(make_int2(c.lo[b * L + l], c.chi[b * L + l]));
        rtab.push_back(make_int2(c.lo[b * L + l], c.ohi[b * L + l]));
      }
    // Per band, the row entries pyr_band_kernel stages in LDS: the computed
    // rows of levels 1 .. L-1 in turn, {sy0 | sy1 << 16, 4*b0 | 4*b1 << 16}
    // (the 2x2 area mean: rows 2r and 2r + 1, 4*b = 2048). The band's level-0
    // own entry, which nothing reads, becomes {the list's offset, its length}.
    for (int b = 0; b < c.nb; ++b) {
      const int at = (int)rtab.size();
      for (int l = 1; l < L; ++l)
        for (int r = c.lo[b * L + l]; r <= c.chi[b * L + l]; ++r) {
          const int2 e = rtab[P.lv[l].ytab + r];
          rtab.push_back(P.lv[l].area2x ? make_int2((2 * r) | ((2 * r + 1) << 16), 2048 | (2048 << 16))
                                        : make_int2(e.x, e.y << 2));
        }
      rtab[q.bands + b * L * 2 + 1] = make_int2(at, (int)rtab.size() - at);
    }
    q.ctiles = (int)rtab.size();
    const PyrCols& C = c.cols;
    auto origin = [&](int t, int l) { return l == 0 ? (C.lo[t * L] & ~15) : C.lo[t * L + l]; };
    for (int t = 0; t < C.nct; ++t)
      for (int l = 0; l < L; ++l) {
        const int lo = C.lo[t * L + l];
        rtab.push_back(make_int2(lo, C.chi[t * L + l]));
        rtab.push_back(make_int2(lo, C.ohi[t * L + l]));
        rtab.push_back(make_int2(C.lpitch[l], origin(t, l)));
        rtab.push_back(make_int2(0, 0));  // .x: the level's column records (below)
      }
    // Column records of pyr_band_kernel, per (tile, level >= 1, column group
    // gi): what a thread's 8 columns need in the row loop, ready for its
    // registers: 24 dwords = the 4 runs' LDS-relative dword-pair offsets, the
    // 8 v_perm_b32 selectors, the 8 {a0 | a1 << 16}, and the store flags (bit
    // k: run k is owned whole by the tile; bit 4 + k: only its first column
    // is, the level's last). None of it depends on the frame, the band or the
    // launch, and worked out per thread and level in the kernel it was the
    // largest share of the kernel's vector instructions.
    // Records start at even int2 indices: 16-byte loads.
    for (int t = 0; t < C.nct; ++t)
      for (int l = 1; l < L; ++l) {
        if (rtab.size() & 1) rtab.push_back(make_int2(0, 0));
        rtab[q.ctiles + (t * L + l) * 4 + 3].x = (int)rtab.size();
        const LevelGeom& g = P.lv[l];
        const int lo = C.lo[t * L + l], ohi = C.ohi[t * L + l];
        const int G = (C.chi[t * L + l] - lo + 1 + 7) >> 3, org = origin(t, l - 1);
        for (int gi = 0; gi < G; ++gi) {
          uint32_t rec[24] = {};
          for (int qq = 0; qq < 8; ++qq) {
            const int col = lo + 2 * (gi + (qq >> 1) * G) + (qq & 1);  // pyr_col
            const int2 e = rtab[g.xtab2 + std::min(col, g.w - 1)];
            const int sx = e.x - org;
            if (!(qq & 1)) rec[qq >> 1] = (uint32_t)(sx & ~3);
            const uint32_t o = (uint32_t)sx - rec[qq >> 1];  // 0 .. 6
            rec[4 + qq] = 0x0c000c00u | o | ((o + 1) << 16);
            rec[12 + qq] = g.area2x ? (2048u | (2048u << 16)) : (uint32_t)e.y;
          }
          for (int k = 0; k < 4; ++k) {
            const int gx = lo + 2 * (gi + k * G);
            if (gx >= lo && gx < ohi) rec[20] |= 1u << k;
            if (gx == ohi) rec[20] |= 16u << k;
          }
          for (int i = 0; i < 24; i += 2) rtab.push_back(make_int2((int)rec[i], (int)rec[i + 1]));
        }
      }
    if (pyr_records_ok(P, rtab, q) < 0) --P.pyr_nplans;
  }
  if (!P.pyr_nplans) return;
  P.pyr_fused = 1;
  select_pyr_plan(P, 0);  // the default; launch_pyramid picks per launch
}

// Path codes of the sorted-key quadtree (orbx_quadtree.hip): a node box of
// DistributeOctTree never depends on the data (roots: nIni columns of width
// hX, src/ORBextractor.cc:903-914; children: DivideNode's ceil halves,
// :833-834), so the quadrant of a key at every depth is a function of its x
// alone (x half) and of its y alone (y half). t = boxW x codes (root index in
// the top bits, x digit at even bits), then boxH y codes (y digit at odd
// bits), Dh digits each: xs[x] | ys[y] is the key's bin, its node at depth
// Dh. bits = 0 (code shift) | Dh << 8 | log2(bins) << 16; bins stay within
// 4096..8192 so that the bin scan keeps 2..8 words per thread.
static bool qt_code_tables(const LevelGeom& g, std::vector<uint32_t>& t, int* bits) {
  int R = 0;
  while ((1 << R) < g.nIni) ++R;
  if (R > 5 || g.boxW < 1 || g.boxH < 1 || g.boxW > 0xFFFF || g.boxH > 0xFFFF) return false;
  const int Dh = (13 - R) / 2;
  t.assign((size_t)g.boxW + g.boxH, 0u);
  for (int x = 0; x < g.boxW; ++x) {
    // vpIniNodes[kp.pt.x/hX] (:920); columns past the last root never hold keys
    const int r = std::min((int)((float)x / g.hX), g.nIni - 1);
    int a = (int)(g.hX * (float)r), c = (int)(g.hX * (float)(r + 1));
    uint32_t code = (uint32_t)r << (2 * Dh);
    for (int j = 0; j < Dh; ++j) {
      const int mid = a + (int)std::ceil((float)(c - a) / 2.f);
      const int bit = x >= mid;
      if (bit) a = mid; else c = mid;
      code |= (uint32_t)bit << (2 * (Dh - 1 - j));
    }
    t[x] = code;
  }
  for (int y = 0; y < g.boxH; ++y) {
    int a = 0, c = g.boxH;
    uint32_t code = 0;
    for (int j = 0; j < Dh; ++j) {
      const int mid = a + (int)std::ceil((float)(c - a) / 2.f);
      const int bit = y >= mid;
      if (bit) a = mid; else c = mid;
      code |= (uint32_t)bit << (2 * (Dh - 1 - j) + 1);
    }
    t[(size_t)g.boxW + y] = code;
  }
  *bits = (Dh << 8) | ((R + 2 * Dh) << 16);
  return true;
}

// The host part of a plan: geometry, tables and tilings. No device call.
int orbx::build_plan_host(const orbx_config& c, const ScaleTables& t, int W, int Hh, int B, HostPlan& pl) {
  const int L = c.nlevels;
  ExtractParams P{};
  P.L = L;
  P.B = B;
  const int ini = std::min(std::max(c.ini_th_fast, 0), 255), mn = std::min(std::max(c.min_th_fast, 0), 255);
  P.t_ini = ini;
  P.t_min = mn;
  P.t_low = std::min(ini, mn);
  P.pattern_upstream = c.pattern_mode == ORBX_PATTERN_UPSTREAM;
  gaussian7(P.gauss);
  pl.cells.clear();
  pl.rtab.clear();
  long long lvl_off = 0;  // level planes [l][B][h][pitch], same offsets in pyramid and blur
  int slot = 0, kbase = 0, maxnodes = 0, maxcells = 0;
  for (int l = 0; l < L; ++l) {
    LevelGeom& g = P.lv[l];
    const float inv = t.inv_scale[l];
    g.w = cv_round((float)W * inv);
    g.h = cv_round((float)Hh * inv);
    if (g.w > kMaxLevelDim || g.h > kMaxLevelDim)
      return g_err.fail(ORBX_EINVAL, "level %d is %dx%d; at most %d px per side", l, g.w, g.h, kMaxLevelDim);
    g.pitch = (g.w + 63) & ~63;
    g.plane = (long long)g.h * g.pitch;
    // FAST grid (src/ORBextractor.cc:1133-1147)
    g.minBX = kEdgeThreshold - 3;
    g.minBY = g.minBX;
    g.maxBX = g.w - kEdgeThreshold + 3;
    g.maxBY = g.h - kEdgeThreshold + 3;
    const float width = (float)(g.maxBX - g.minBX), height = (float)(g.maxBY - g.minBY);
    g.nCols = (int)(width / kGridW);
    g.nRows = (int)(height / kGridW);
    if (g.nCols < 1 || g.nRows < 1)
      return g_err.fail(ORBX_EINVAL,
                  "level %d (%dx%d) is smaller than one %d-px FAST cell inside the %d-px border; "
                  "the reference divides by zero here (src/ORBextractor.cc:1144-1147)",
                  l, g.w, g.h, kGridW, kEdgeThreshold);
    g.wCell = (int)std::ceil(width / g.nCols);
    g.hCell = (int)std::ceil(height / g.nRows);
    if (g.wCell + 6 > kMaxRoi - 1 || g.hCell + 6 > kMaxRoi - 1)
      return g_err.fail(ORBX_EINVAL, "level %d cell %dx%d exceeds the ROI tile", l, g.wCell, g.hCell);
    g.cell0 = (int)pl.cells.size();
    g.slot0 = slot;
    for (int i = 0; i < g.nRows; i++) {
      const float iniY = g.minBY + i * g.hCell;
      float maxY = iniY + g.hCell + 6;
      const bool skipRow = iniY >= g.maxBY - 3;
      if (maxY > g.maxBY) maxY = g.maxBY;
      for (int j = 0; j < g.nCols; j++) {
        const float iniX = g.minBX + j * g.wCell;
        float maxX = iniX + g.wCell + 6;
        const bool skip = skipRow || iniX >= g.maxBX - 6;
        if (maxX > g.maxBX) maxX = g.maxBX;
        CellGeom cg{};
        cg.level = (int16_t)l;
        cg.c0 = (int16_t)(int)iniX;
        cg.r0 = (int16_t)(int)iniY;
        cg.c1 = (int16_t)(int)maxX;
        cg.r1 = (int16_t)(int)maxY;
        const int bw = cg.c1 - cg.c0 - 6, bh = cg.r1 - cg.r0 - 6;
        cg.cap = (skip || bw <= 0 || bh <= 0) ? 0 : (int16_t)(((bw + 1) / 2) * ((bh + 1) / 2));
        if (cg.cap) {
          P.fast_rh_max = std::max(P.fast_rh_max, cg.r1 - cg.r0);
          P.fast_bw_max = std::max(P.fast_bw_max, bw);
          P.fast_bh_max = std::max(P.fast_bh_max, bh);
        }
        cg.pitch = l == 0 ? 0 : g.pitch;
        cg.row_off = l == 0 ? cg.r0 : (int)(lvl_off + (long long)cg.r0 * g.pitch);
        cg.fstride = l == 0 ? 0 : (int)g.plane;
        cg.geo = (g.h - 1 - cg.r0) | (((g.w + 15) & ~15) << 16);
        pl.cells.push_back(cg);
      }
    }
    g.ncells = (int)pl.cells.size() - g.cell0;
    // slot ranges at one stride per level (the largest cell's NMS bound):
    // cell c's keys start at slot0 + c * stride, so the sorted quadtree
    // finds them without reading the cell records
    int stride = 1;
    for (int c = g.cell0; c < (int)pl.cells.size(); ++c) stride = std::max(stride, (int)pl.cells[c].cap);
    for (int c = g.cell0; c < (int)pl.cells.size(); ++c) pl.cells[c].slot_off = slot + (c - g.cell0) * stride;
    g.slot_stride = stride;
    slot += g.ncells * stride;
    g.nslots = slot - g.slot0;
    maxcells = std::max(maxcells, g.ncells);
    // DistributeOctTree (src/ORBextractor.cc:894-898)
    g.N = t.nfeat[l];
    g.boxW = g.maxBX - g.minBX;
    g.boxH = g.maxBY - g.minBY;
    g.nIni = (int)roundf(static_cast<float>(g.boxW) / g.boxH);
    if (g.nIni < 1) return g_err.fail(ORBX_EINVAL, "level %d: nIni = 0 (image taller than 1.5x its width)", l);
    g.hX = static_cast<float>(g.boxW) / g.nIni;
    g.kcap = std::max(g.N + 3, g.nIni);
    g.kbase = kbase;
    // levels start at multiples of kKpGroup slots, so an orient+BRIEF
    // workgroup's keypoints all sit in one level
    kbase += (g.kcap + kKpGroup - 1) / kKpGroup * kKpGroup;
    maxnodes = std::max(maxnodes, g.kcap + 4);
    g.scale = t.scale[l];
    g.size = (float)(int)(kPatchSize * t.scale[l]);
    g.off = lvl_off;
    lvl_off += (long long)B * g.plane;
    if (l >= 1) {
      std::vector<int2> xt, yt;
      resize_tables(P.lv[l - 1].w, P.lv[l - 1].h, g.w, g.h, xt, yt, &g.xmax, &g.area2x);
      // the pyramid kernel stages each 16 x 256 output tile's source footprint
      // in a 36 x 576 LDS tile (orbx_pyramid.hip): true for scaleFactor <= 2
      for (int x0 = 0; x0 < g.w; x0 += 256) {
        const int xe = std::min(x0 + 255, g.w - 1);
        const int lo = g.area2x ? 2 * x0 : xt[x0].x, hi = g.area2x ? 2 * xe + 1 : xt[xe].x + 1;
        if (hi - (lo & ~15) + 16 > 576)
          return g_err.fail(ORBX_EINVAL, "scaleFactor %g too large for the pyramid tile (max 2.0)", c.scale_factor);
      }
      for (int y0 = 0; y0 < g.h; y0 += 16) {
        const int ye = std::min(y0 + 15, g.h - 1);
        const int lo = g.area2x ? 2 * y0 : (yt[y0].x & 0xFFFF), hi = g.area2x ? 2 * ye + 1 : (yt[ye].x >> 16);
        if (hi - lo + 1 > 36)
          return g_err.fail(ORBX_EINVAL, "scaleFactor %g too large for the pyramid tile (max 2.0)", c.scale_factor);
      }
      g.xtab = (int)pl.rtab.size();
      pl.rtab.insert(pl.rtab.end(), xt.begin(), xt.end());
      g.ytab = (int)pl.rtab.size();
      pl.rtab.insert(pl.rtab.end(), yt.begin(), yt.end());
      // band-pyramid column table: columns at or past xmax replicate S[sx]
      // (x2048), the same as coefficients {2048, 0}
      g.xtab2 = (int)pl.rtab.size();
      for (int dx = 0; dx < g.w; ++dx) {
        int2 e = xt[dx];
        if (g.area2x) e = make_int2(2 * dx, 0);
        else if (dx >= g.xmax) e.y = 2048;
        pl.rtab.push_back(e);
      }
    }
  }
  // sorted-key quadtree: per level, the depth-Dh path code of every column
  // (root index on top) and of every row (orbx_quadtree.hip), two u32 per
  // int2 of the resize table
  P.qt_tabmax = 0;
  P.qt_nbmax = 0;
  for (int l = 0; l < L; ++l) {
    LevelGeom& g = P.lv[l];
    std::vector<uint32_t> t;
    int bits = 0;
    g.qt_tab = -1;
    if (qt_code_tables(g, t, &bits)) {
      g.qt_tab = (int)pl.rtab.size() * 2;
      g.qt_dims = g.boxW | (g.boxH << 16);
      g.qt_bits = bits;
      if (t.size() & 1) t.push_back(0u);
      for (size_t i = 0; i < t.size(); i += 2) pl.rtab.push_back(make_int2((int)t[i], (int)t[i + 1]));
      P.qt_tabmax = std::max(P.qt_tabmax, g.boxW + g.boxH);
      P.qt_nbmax = std::max(P.qt_nbmax, 1 << ((bits >> 16) & 0xFF));
    }
  }
  if (lvl_off > INT_MAX)  // FAST's cell records hold 32-bit plane offsets
    return g_err.fail(ORBX_EINVAL, "max_batch %d: the pyramid planes take %lld bytes, over 2 GiB", B, lvl_off);
  plan_band_pyramid(P, pl.rtab);
  for (int v = 0; v < 2; ++v) {
    // blur work lists, long and short segments (orbx_blur.hip): one entry per
    // wave, level-major, a strip's segments top to bottom, so the four waves
    // of a workgroup mostly share their halo rows
    int sw = 0, R = 0;
    blur_strip_dims(v, &sw, &R);
    P.blur_tiles[v] = (int)pl.rtab.size();
    for (int l = 0; l < L; ++l)
      for (int x0 = 0; x0 < P.lv[l].w; x0 += sw)
        for (int y0 = 0; y0 < P.lv[l].h; y0 += R)
          pl.rtab.push_back(make_int2(l | (x0 << 4) | (y0 << 16), std::min(R, P.lv[l].h - y0)));
    P.blur_ntiles[v] = (int)pl.rtab.size() - P.blur_tiles[v];
    P.blur_magic[v] = exact_div_magic((unsigned long long)(P.blur_ntiles[v] + 3) / 4, B);  // workgroups per frame
  }
  if (maxnodes > 65000) return g_err.fail(ORBX_EINVAL, "nfeatures too large for the quadtree node table");
  P.slots_per_frame = slot;
  P.ncells_total = (int)pl.cells.size();
  P.ncells_magic = exact_div_magic(P.ncells_total, B);  // FAST's frame index without a division
  P.kp_per_frame = kbase;
  P.maxnodes = maxnodes;
  int sn = 1;
  while (sn < maxnodes) sn <<= 1;
  P.sortn = sn;
  P.max_cells_level = maxcells;
  P.kcap_lds = 0;
  {
    const char* e = getenv("ORBX_QT_GENERIC");  // tests: the generic rounds on any plan
    P.qt_lean = maxnodes < 16384 && !(e && e[0] == '1');
    // the sorted-key path first (ORBX_QT_SORTED=0: the legacy rounds only, for A/B and tests)
    const char* so = getenv("ORBX_QT_SORTED");
    P.qt_sorted = P.qt_lean && P.qt_nbmax > 0 && !(so && so[0] == '0');
  }
  {
    // keep the LDS footprint at 80 KiB so two quadtree blocks fit one CU,
    // unless the node tables alone nearly fill that (large levels: 1920x1080
    // has 102 KB of them). Then a block takes a whole CU: 1024 threads (its
    // key passes, which set its time there, on twice the lanes) and 160 KiB,
    // the rest of it for keys
#ifndef ORBX_QT_LDS_KB
#define ORBX_QT_LDS_KB 80
#endif
    const size_t base = quadtree_legacy_lds_bytes(P);
    size_t small = ORBX_QT_LDS_KB * 1024, big = 160 * 1024 - 512;
    if (const char* e = getenv("ORBX_QT_LDS_KB")) small = (size_t)std::max(32, atoi(e)) * 1024;  // A/B: blocks per CU
    P.qt_big = base + 16 * 1024 > small ? 1 : 0;
    const size_t budget = P.qt_big ? big : small;
    P.kcap_lds = base < budget ? (int)((budget - base) / 6) & ~15 : 0;
    // the sorted path shares the block's LDS (its layout is the legacy one's
    // alternative, not an addition): on when it fits the same budget
    if (P.qt_sorted) {
      P.qt_ownmax = quadtree_sorted_ownmax(P, P.qt_big, budget);
      if (!P.qt_ownmax || quadtree_sorted_lds_bytes(P, P.qt_big) > budget) P.qt_sorted = 0;
    }
    // the sorted path's rounds hold two nodes per thread
    if (maxnodes > 2 * (P.qt_big ? 1024 : kQtThreads)) P.qt_sorted = 0;
    if (getenv("ORBX_PLAN_INFO"))  // diagnostics: the quadtree block's LDS per path
      fprintf(stderr,
              "plan %dx%d B %d: quadtree LDS legacy %zu sorted %zu (budget %zu) sorted %d big %d maxnodes %d "
              "nbmax %d tabmax %d ownmax %d\n",
              W, Hh, B, base, P.qt_nbmax ? quadtree_sorted_lds_bytes(P, P.qt_big) : (size_t)0, budget, P.qt_sorted,
              P.qt_big, maxnodes, P.qt_nbmax, P.qt_tabmax, P.qt_ownmax);
  }
  pl.P = P;
  pl.W = W;
  pl.H = Hh;
  pl.B = B;
  pl.level_bytes = lvl_off;
  return ORBX_OK;
}

extern "C" {

/* Internal, for the tests (not part of orbx_c.h, needs no device): plans `cfg`
 * on the host and checks the band pyramid's column records of every kept plan
 * (pyr_records_ok). *nplans: the kept plans (0: the per-level kernel runs);
 * records[i]: plan i's records checked, -1 if a bound fails. */
int orbx_pyr_plan_check(const orbx_config* cfg, long long* records, int cap, int* nplans) {
  if (!cfg || !records || !nplans) return g_err.fail(ORBX_EINVAL, "null argument");
  if (cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || !(cfg->scale_factor > 1.0f) || cfg->width <= 0 ||
      cfg->height <= 0 || cfg->max_batch < 1)
    return g_err.fail(ORBX_EINVAL, "bad configuration");
  ScaleTables t;
  HostPlan pl;
  compute_scales(*cfg, t);
  const int rc = build_plan_host(*cfg, t, cfg->width, cfg->height, cfg->max_batch, pl);
  if (!rc) {
    const ExtractParams& P = pl.P;
    *nplans = P.pyr_fused ? P.pyr_nplans : 0;
    for (int i = 0; i < *nplans && i < cap; ++i) records[i] = pyr_records_ok(P, pl.rtab, P.pyr_plan[i]);
  }
  return rc;
}

}  // extern "C"

// ------------------------------------------------------------ plan digest
// FNV-1a over the plan's values, field by field (no padding byte is read).
namespace {
struct Fnv {
  unsigned long long h = 1469598103934665603ull;
  size_t fed = 0;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    fed += n;
  }
  template <class T>
  void operator()(const T& v) { bytes(&v, sizeof v); }
};
static_assert(sizeof(LevelGeom) == 152 && sizeof(ExtractParams) == 2920, "a new field: add it to plan_digest");

bool plan_digest(const ExtractParams& P, const std::vector<CellGeom>& cells, const std::vector<int2>& rtab,
                 unsigned long long out[3]) {
  Fnv f;
  f(P.L), f(P.B), f(P.t_low), f(P.t_ini), f(P.t_min), f(P.slots_per_frame), f(P.ncells_total), f(P.ncells_magic);
  f(P.kp_per_frame), f(P.maxnodes), f(P.sortn), f(P.max_cells_level), f(P.kcap_lds), f(P.qt_lean), f(P.qt_big);
  f(P.qt_sorted), f(P.qt_tabmax), f(P.qt_nbmax), f(P.qt_ownmax), f(P.fast_rh_max), f(P.fast_bw_max), f(P.fast_bh_max);
  f(P.pattern_upstream), f(P.pyr_fused), f(P.pyr_nbands), f(P.pyr_bands), f(P.pyr_nct), f(P.pyr_ctiles);
  f(P.pyr_lds_a), f(P.pyr_lds_b), f(P.pyr_lds_y);
  for (const ExtractParams::PyrPlan& q : P.pyr_plan)
    f(q.nbands), f(q.nct), f(q.bands), f(q.ctiles), f(q.lds_a), f(q.lds_b), f(q.lds_y), f(q.cost), f(q.occ);
  f(P.pyr_nplans), f(P.gauss), f(P.blur_tiles), f(P.blur_ntiles), f(P.blur_magic);
  for (const LevelGeom& g : P.lv) {
    f(g.w), f(g.h), f(g.pitch), f(g.plane), f(g.off), f(g.xtab), f(g.ytab), f(g.xmax), f(g.area2x);
    f(g.minBX), f(g.minBY), f(g.maxBX), f(g.maxBY), f(g.nCols), f(g.nRows), f(g.wCell), f(g.hCell);
    f(g.cell0), f(g.ncells), f(g.slot0), f(g.nslots), f(g.slot_stride), f(g.N), f(g.nIni), f(g.boxW), f(g.boxH);
    f(g.hX), f(g.kcap), f(g.kbase), f(g.scale), f(g.size), f(g.xtab2), f(g.qt_tab), f(g.qt_dims), f(g.qt_bits);
  }
  // everything but the 4 padding bytes of each level and before them, and the two status pointers
  if (f.fed != sizeof(ExtractParams) - 4 * (kMaxLevels + 1) - 2 * sizeof(void*) || P.status_src || P.status_dst)
    return false;
  out[0] = f.h;
  Fnv c, r;
  c.bytes(cells.data(), cells.size() * sizeof(CellGeom));  // CellGeom has no padding (32 bytes of fields)
  r.bytes(rtab.data(), rtab.size() * sizeof(int2));
  out[1] = c.h;
  out[2] = r.h;
  return true;
}
}  // namespace

/* Internal, for the tests (not part of orbx_c.h, needs no device): plans `cfg`
 * on the host as orbx_create does and returns FNV-1a digests of the parameter
 * block, the cell table and the resize table. */
extern "C" int orbx_plan_digest(const orbx_config* cfg, unsigned long long out[3]) {
  if (!cfg || !out) return g_err.fail(ORBX_EINVAL, "null argument");
  if (cfg->nlevels < 1 || cfg->nlevels > kMaxLevels || !(cfg->scale_factor > 1.0f) || cfg->width <= 0 ||
      cfg->height <= 0 || cfg->max_batch < 1)
    return g_err.fail(ORBX_EINVAL, "bad configuration");
  ScaleTables t;
  HostPlan pl;
  compute_scales(*cfg, t);
  const int rc = build_plan_host(*cfg, t, cfg->width, cfg->height, cfg->max_batch, pl);
  if (rc) return rc;
  return plan_digest(pl.P, pl.cells, pl.rtab, out) ? ORBX_OK : g_err.fail(ORBX_EINVAL, "plan digest: field list out of date");
}

/* Internal: exact_div_magic, for the test of FAST's frame index. */
extern "C" unsigned orbx_exact_div_magic(unsigned long long d, unsigned long long batch) {
  return exact_div_magic(d, batch);
}
