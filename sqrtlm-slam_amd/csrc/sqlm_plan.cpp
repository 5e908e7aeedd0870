// sqlm_plan.cpp — the host-only planner of a BA setup (see sqlm_plan.h):
// initializeOptimization(level) + BlockSolver::buildStructure as stages.
// No HIP call: it builds with a plain C++ compiler (tools/plan_check.cpp).
#include "sqlm_plan.h"

#include <limits>
#include <queue>

namespace sqlm {

void build_tiles(int nP, int nL, const std::vector<int> &lm_begin, const int *obs_camh, int lm_cap, TilePlan &tp,
                 TileBuild &tb, int *obs_local) {
  const int64_t nE = lm_begin[nL];
  PhaseTimer sub(kPhaseTiles);
  tp.reset();
  tp.urange.assign(nL, int2{-1, -1});
  // pass 1 (greedy): tile boundaries -- a tile closes before the landmark that
  // would push its window past kTileMaxCams cameras or lm_cap. The slots are
  // cut into a number of chunks that depends on the problem only (one per
  // 128k observations, at most 16; a tile never crosses a chunk start), so the
  // tile plan -- and with it the fixed summation order of S -- is the same on
  // every host; the chunks are then dealt to however many threads there are.
  std::vector<int> &tstart = tb.tstart;
  tstart.clear();
  {
    const int nchunk = (int)std::max<int64_t>(1, std::min<int64_t>(16, nE / 131072));
    const int nth = std::min(nchunk, host_threads(nE));
    std::vector<std::vector<int>> cuts(nchunk);
    std::vector<uint8_t> dup(nchunk, 0);
    run_threads(nth, [&](int th) {
      std::vector<int> stamp(nP, -1), lmst(nP, -1);
      for (int ch = th; ch < nchunk; ch += nth) {
        const int s0 = (int)((int64_t)nL * ch / nchunk), s1 = (int)((int64_t)nL * (ch + 1) / nchunk);
        std::vector<int> &cv = cuts[ch];
        int t = 0, ncur = 0, cur_lm = 0;
        std::fill(stamp.begin(), stamp.end(), -1);
        for (int sl = s0; sl < s1; ++sl) {
          int nnew = 0;
          for (int o = lm_begin[sl]; o < lm_begin[sl + 1]; ++o) {
            const int h = obs_camh[o];
            if (h < 0) continue;
            if (lmst[h] == sl) { dup[ch] = 1; continue; }
            lmst[h] = sl;
            if (stamp[h] != t) ++nnew;
          }
          if (cur_lm == 0 || ncur + nnew > kTileMaxCams || cur_lm >= lm_cap) {
            cv.push_back(sl);
            ++t;
            ncur = 0;
            cur_lm = 0;
          }
          for (int o = lm_begin[sl]; o < lm_begin[sl + 1]; ++o) {
            const int h = obs_camh[o];
            if (h >= 0 && stamp[h] != t) { stamp[h] = t; ++ncur; }
          }
          ++cur_lm;
        }
      }
    });
    for (int ch = 0; ch < nchunk; ++ch) {
      tstart.insert(tstart.end(), cuts[ch].begin(), cuts[ch].end());
      if (dup[ch]) tp.dups = true;
    }
    if (tstart.empty() || tstart[0] != 0) tstart.insert(tstart.begin(), 0);
    if (nL > 0) tstart.push_back(nL);
    else tstart.assign(1, 0);
  }
  sub("pass 1");
  const int nt = (int)tstart.size() - 1;
  // pass 2 (tiles on host threads): window cameras, local camera of every
  // observation, landmark spans, and the S blocks each tile contributes to
  std::vector<TileBuild::TileOut> &out = tb.out;
  out.assign(nt, TileBuild::TileOut{});
  const int nth = host_threads(nE);
  run_threads(nth, [&](int th) {
    std::vector<int> lidx(nP, -1), lcams;
    std::vector<uint8_t> pst;
    std::vector<uint64_t> rowm;
    for (int t = th; t < nt; t += nth) {
      // the window's cameras: first sight marks (lidx = -2), then sorted (<= 24 of them)
      std::vector<int> &cur = out[t].cams;
      for (int o = lm_begin[tstart[t]]; o < lm_begin[tstart[t + 1]]; ++o) {
        const int h = obs_camh[o];
        if (h >= 0 && lidx[h] == -1) { lidx[h] = -2; cur.push_back(h); }
      }
      std::sort(cur.begin(), cur.end());
      const int cp = (int)cur.size();
      for (int u = 0; u < cp; ++u) lidx[cur[u]] = u;
      // co-observed camera pairs (u <= v): as one bit row per camera when the
      // window fits 64 (a landmark ORs its camera set into the rows of its
      // cameras: linear in its track, not quadratic), else as a byte matrix
      const bool bits = cp <= 64;
      if (bits) rowm.assign(cp, 0);
      else pst.assign((size_t)cp * cp, 0);
      for (int sl = tstart[t]; sl < tstart[t + 1]; ++sl) {
        lcams.clear();
        int lo = cp, hi = -1;
        uint64_t set = 0;
        for (int o = lm_begin[sl]; o < lm_begin[sl + 1]; ++o) {
          const int h = obs_camh[o];
          const int u = h >= 0 ? lidx[h] : -1;
          obs_local[o] = u;
          if (u >= 0) {
            lcams.push_back(u);
            lo = std::min(lo, u);
            hi = std::max(hi, u);
            if (bits) set |= uint64_t(1) << u;
          }
        }
        if (hi < 0) continue;
        tp.urange[sl] = int2{lo, hi};
        if (bits) {
          for (const int u : lcams) rowm[u] |= set;
          continue;
        }
        const size_t m = lcams.size();  // (a repeated camera only marks its pairs twice)
        for (size_t a = 0; a < m; ++a)
          for (size_t b = a; b < m; ++b) {
            const int u = std::min(lcams[a], lcams[b]), v = std::max(lcams[a], lcams[b]);
            pst[(size_t)u * cp + v] = 1;
          }
      }
      for (int u = 0; u < cp; ++u)
        for (int v = u; v < cp; ++v)
          if (bits ? (rowm[u] >> v & 1) : pst[(size_t)u * cp + v])
            out[t].red.push_back({cur[u], t, tile_blk(u, v, cp), cur[v]});
      for (int u = 0; u < cp; ++u) lidx[cur[u]] = -1;
    }
  });
  sub("pass 2");
}

// S pattern (upper, diagonal first) of the free cameras from the tiles'
// camera pairs: every pair of cameras that co-observe a landmark is marked in
// the tile that holds the landmark; plus every diagonal.
void pattern_from_tiles(int nP, const TileBuild &tb, std::vector<int> &s_row, std::vector<int> &s_col) {
  const int nt = (int)tb.out.size();
  const int nth = host_threads((int64_t)nt * 256);
  std::vector<std::vector<int>> cnt(nth, std::vector<int>(nP, 0));
  run_threads(nth, [&](int th) {
    for (int t = th; t < nt; t += nth)
      for (const auto &r : tb.out[t].red)
        if (r.j != r.key) ++cnt[th][r.key];
  });
  std::vector<int> ptr(nP + 1, 0);
  for (int i = 0; i < nP; ++i) {
    int b = ptr[i] + 1;  // the diagonal first
    for (int th = 0; th < nth; ++th) { const int k = cnt[th][i]; cnt[th][i] = b; b += k; }
    ptr[i + 1] = b;
  }
  std::vector<int> raw(ptr[nP]);
  for (int i = 0; i < nP; ++i) raw[ptr[i]] = i;
  run_threads(nth, [&](int th) {
    for (int t = th; t < nt; t += nth)
      for (const auto &r : tb.out[t].red)
        if (r.j != r.key) raw[cnt[th][r.key]++] = r.j;
  });
  std::vector<int> len(nP);
  // (sorting is heavier per entry than a copy: more threads than a pass would take)
  run_threads(host_threads(8 * (int64_t)ptr[nP]), [&](int th) {
    const int n = host_threads(8 * (int64_t)ptr[nP]);
    for (int i = (int)((int64_t)nP * th / n); i < (int)((int64_t)nP * (th + 1) / n); ++i) {
      int *b = raw.data() + ptr[i] + 1, *e = raw.data() + ptr[i + 1];
      std::sort(b, e);
      len[i] = 1 + (int)(std::unique(b, e) - b);
    }
  });
  s_row.assign(nP + 1, 0);
  for (int i = 0; i < nP; ++i) s_row[i + 1] = s_row[i] + len[i];
  s_col.resize(s_row[nP]);
  for (int i = 0; i < nP; ++i) std::copy(raw.begin() + ptr[i], raw.begin() + ptr[i] + len[i], s_col.begin() + s_row[i]);
}

// The reduction lists of the tiles (needs the final S pattern).
void build_tiles_finish(int nP, const std::vector<int> &s_row, const std::vector<int> &s_col, TilePlan &tp,
                        TileBuild &tb) {
  PhaseTimer sub(kPhaseTiles);
  using Red = TileBuild::Red;
  std::vector<TileBuild::TileOut> &out = tb.out;
  const std::vector<int> &tstart = tb.tstart;
  const int nt = (int)out.size();
  run_threads(host_threads((int64_t)nt * 256), [&](int th) {  // S block of every tile pair
    const int n = host_threads((int64_t)nt * 256);
    for (int t = th; t < nt; t += n)
      for (Red &r : out[t].red) {
        const int *b0 = s_col.data() + s_row[r.key], *b1 = s_col.data() + s_row[r.key + 1];
        r.key = (int)(std::lower_bound(b0, b1, r.j) - s_col.data());
      }
  });
  sub("keys");
  // pass 3 (tile order): offsets, camera lists, the reduction lists (the
  // lists concatenated on host threads at per-tile offsets)
  std::vector<Red> red, gred;
  {
    std::vector<size_t> roff(nt + 1, 0), goff(nt + 1, 0);
    for (int t = 0; t < nt; ++t) {
      roff[t + 1] = roff[t] + out[t].red.size();
      goff[t + 1] = goff[t] + out[t].cams.size();
    }
    red.resize(roff[nt]);
    gred.resize(goff[nt]);
    const int nr = host_threads((int64_t)roff[nt]);
    run_threads(nr, [&](int th) {
      for (int t = (int)((int64_t)nt * th / nr); t < (int)((int64_t)nt * (th + 1) / nr); ++t) {
        std::copy(out[t].red.begin(), out[t].red.end(), red.begin() + roff[t]);
        for (size_t u = 0; u < out[t].cams.size(); ++u) gred[goff[t] + u] = Red{out[t].cams[u], t, (int)u, 0};
      }
    });
  }
  for (int t = 0; t < nt; ++t) {
    const std::vector<int> &cur = out[t].cams;
    const int cp = (int)cur.size();
    const int ld = (6 * cp + 15) / 16 * 16;
    tp.ld.push_back(ld);
    tp.part_ptr.push_back(tp.part_ptr.back() + 36 * (int64_t)(cp * (cp + 1) / 2));
    tp.gpart_ptr.push_back(tp.gpart_ptr.back() + ld);
    tp.cams.insert(tp.cams.end(), cur.begin(), cur.end());
    tp.cam_ptr.push_back(tp.cam_ptr.back() + cp);
    tp.lm_ptr.push_back(tstart[t + 1]);
    tp.max_cp = std::max(tp.max_cp, cp);
  }
  {  // launch classes by accumulator width
    std::vector<int> cls(nt);
    bool any4 = false;
    for (int t = 0; t < nt; ++t) any4 |= (6 * (int)out[t].cams.size() + 15) / 16 == 4;
    for (int t = 0; t < nt; ++t) {
      // classes 3 (only when no tile needs 4: small windows, e.g. local BA), 4,
      // 6, 8, 9 — a tile goes to the narrowest one that holds it; the odd widths
      // hold a few dozen tiles each, too few for a launch of their own
      const int w = (6 * (int)out[t].cams.size() + 15) / 16;
      cls[t] = w <= 3 && !any4 ? 3 : w <= 4 ? 4 : w <= 6 ? 6 : w <= 8 ? 8 : kTileNtMax;
      tp.cls_cnt[cls[t]]++;
    }
    tp.cls_off[0] = 0;
    for (int k = 0; k <= kTileNtMax; ++k) tp.cls_off[k + 1] = tp.cls_off[k] + tp.cls_cnt[k];
    tp.order.assign(std::max(nt, 1), 0);
    std::vector<int> f(tp.cls_off, tp.cls_off + kTileNtMax + 1);
    for (int t = 0; t < nt; ++t) tp.order[f[cls[t]]++] = t;
  }
  if (sub.on) {  // window widths of the tiles (cameras), for the NT classes
    int hist[kTileHardCams + 2] = {0};
    for (int t = 0; t < nt; ++t) hist[std::min((int)out[t].cams.size(), kTileHardCams + 1)]++;
    std::fprintf(stderr, "sqlm tiles: %d, cameras per window:", nt);
    for (int c = 0; c <= kTileHardCams + 1; ++c)
      if (hist[c]) std::fprintf(stderr, " %d:%d", c, hist[c]);
    std::fprintf(stderr, "\n");
  }
  sub("pass 3");
  auto csr = [](const std::vector<Red> &v, int nkeys, std::vector<int> &ptr, std::vector<int2> &idx) {
    ptr.assign(nkeys + 1, 0);
    for (auto &r : v) ptr[r.key + 1]++;
    for (int k = 0; k < nkeys; ++k) ptr[k + 1] += ptr[k];
    idx.resize(v.size());
    std::vector<int> f(ptr.begin(), ptr.end() - 1);
    for (auto &r : v) idx[f[r.key]++] = int2{r.tile, r.code};
  };
  std::vector<int2> red_idx;
  csr(red, s_row[nP], tp.red_ptr, red_idx);
  tp.red_off.resize(red_idx.size());
  {
    const int64_t n = (int64_t)red_idx.size();
    const int nc = host_threads(n);
    run_threads(nc, [&](int t) {
      for (int64_t k = n * t / nc; k < n * (t + 1) / nc; ++k)
        tp.red_off[k] = tp.part_ptr[red_idx[k].x] + 36 * (int64_t)red_idx[k].y;
    });
  }
  csr(gred, nP, tp.gred_ptr, tp.gred_idx);
  tp.gred_off.resize(tp.gred_idx.size());
  for (size_t k = 0; k < tp.gred_idx.size(); ++k)
    tp.gred_off[k] = tp.gpart_ptr[tp.gred_idx[k].x] + 6 * (int64_t)tp.gred_idx[k].y;
  for (int s = 0; s < s_row[nP]; ++s)
    if (tp.red_ptr[s + 1] - tp.red_ptr[s] > kRedLong) tp.long_s.push_back(s);
  for (int i = 0; i < nP; ++i)
    if (tp.gred_ptr[i + 1] - tp.gred_ptr[i] > kRedLong) tp.long_g.push_back(i);
  sub("reduction csr");
}

// Reduced-camera-system solver plan from the upper block pattern of S (hidx
// order; SimplicialLDLT + AMD in the reference, linear_solver_eigen.h:60-75).
// Blocks within kBandMaxCams of the diagonal form the band, solved by cyclic
// reduction over superblocks of B = bandwidth + 1 cameras. Blocks farther off
// (loop closures) are covered by a greedy maximum-degree vertex cover; those
// cameras become the dense border, eliminated last (launch_arrow_solve). The
// cyclic reduction carries the band-border coupling only in the superblocks
// that can hold it: per level, the odd superblocks whose right-hand side is
// nonzero form Z = Linv G, the even ones next to them take the update.
// Returns false when S should go to the dense solver (border too large).
// Superblock width of a band-only S. Any B > bandwidth keeps S
// block-tridiagonal; a wider superblock means fewer cyclic-reduction levels and
// a longer factor chain per level. On small systems (a few superblocks) every
// level is latency -- a factor launch whose diagonal chain grows with n / 16,
// an update and a back-substitution launch -- so the estimate below (us per
// launch, measured: tools/cr_bench and the local-BA solve trace,
// profiles/r03/solve_trace_lba.txt) picks the cheapest B, ties to the
// narrowest. Larger systems keep B = bandwidth + 1 (their first levels are
// throughput-bound). SQLM_CR_B_MIN=1: always the narrowest (A/B only).
int cr_superblock_width(int bmin, int nband) {
  const bool keep = std::getenv("SQLM_CR_B_MIN") != nullptr;  // read per plan: tests switch it
  if (const char *fb = std::getenv("SQLM_CR_B")) {  // a fixed width (A/B of the estimate only)
    const int b = std::atoi(fb);
    if (b >= bmin && 6 * b <= kCRMaxN) return std::min(b, std::max(nband, 1));
  }
  auto cost = [&](int B) {
    const int nt = (6 * B + 15) / 16, p = (nband + B - 1) / B;
    int L = 0;
    while ((1 << L) < p) ++L;
    return (L + 1) * (2.0 + 2.6 * nt) + L * 5.5 + (L + 1) * 5.0;
  };
  if (keep || bmin <= 0 || (nband + bmin - 1) / bmin > 16) return bmin;
  int best = bmin;
  for (int B = bmin + 1; 6 * B <= kCRMaxN && B <= nband; ++B)
    if (cost(B) < cost(best) - 1e-9) best = B;
  return best;
}

bool plan_rcs(int nP, const std::vector<int> &s_row, const std::vector<int> &s_col, CRPlan &pl,
              std::vector<int> &cam_pos) {
  pl = CRPlan{};
  cam_pos.resize(nP);
  for (int i = 0; i < nP; ++i) cam_pos[i] = i;
  if (nP == 0) return false;
  std::vector<int> lptr(nP + 1, 0), ladj;
  std::vector<std::pair<int, int>> longe;
  for (int i = 0; i < nP; ++i)
    for (int k = s_row[i]; k < s_row[i + 1]; ++k)
      if (s_col[k] - i > kBandMaxCams) longe.emplace_back(i, s_col[k]);
  std::vector<uint8_t> border(nP, 0);
  int nbc = 0;
  if (!longe.empty()) {
    for (auto &e : longe) { ++lptr[e.first + 1]; ++lptr[e.second + 1]; }
    for (int i = 0; i < nP; ++i) lptr[i + 1] += lptr[i];
    ladj.resize(lptr[nP]);
    std::vector<int> fill(lptr.begin(), lptr.end() - 1), deg(nP, 0);
    for (auto &e : longe) { ladj[fill[e.first]++] = e.second; ladj[fill[e.second]++] = e.first; }
    std::priority_queue<std::pair<int, int>> pq;  // (remaining long blocks, camera): ties -> higher index
    for (int i = 0; i < nP; ++i) {
      deg[i] = lptr[i + 1] - lptr[i];
      if (deg[i]) pq.emplace(deg[i], i);
    }
    while (!pq.empty()) {
      const auto [dg, v] = pq.top();
      pq.pop();
      if (border[v] || dg != deg[v] || dg == 0) continue;
      border[v] = 1;
      ++nbc;
      for (int k = lptr[v]; k < lptr[v + 1]; ++k) {
        const int u = ladj[k];
        if (!border[u] && deg[u] > 0) pq.emplace(--deg[u], u);
      }
      deg[v] = 0;
    }
  }
  const int nband = nP - nbc;
  if (nbc > 0) {
    if (nband == 0 || 3 * nbc > nP) return false;
    int pos = 0, b = 0;
    for (int i = 0; i < nP; ++i) cam_pos[i] = border[i] ? -1 - b++ : pos++;
  }
  int bw = 0;
  for (int i = 0; i < nP; ++i)
    for (int k = s_row[i]; k < s_row[i + 1]; ++k)
      if (cam_pos[i] >= 0 && cam_pos[s_col[k]] >= 0) bw = std::max(bw, cam_pos[s_col[k]] - cam_pos[i]);
  int B = std::min(bw + 1, std::max(nband, 1));
  if (nbc == 0) B = cr_superblock_width(B, nband);
  const int n = (6 * B + 15) / 16 * 16;
  if (n > kCRMaxN) return false;
  pl.enabled = true;
  pl.B = B;
  pl.p = (nband + B - 1) / B;
  pl.n = n;
  pl.nband = nband;
  if (nbc == 0) {
    pl.lo = std::getenv("SQLM_CR_LO0") ? 0 : 1;  // read per plan: tests switch it
    return true;
  }
  pl.nbc = nbc;
  pl.R = (6 * nbc + 15) / 16 * 16;
  pl.Rp = (pl.R + kCRMaxN - 1) / kCRMaxN * kCRMaxN;
  // superblocks holding band-border blocks, then the per-level lists
  std::vector<uint8_t> act(pl.p, 0);
  for (int i = 0; i < nP; ++i)
    for (int k = s_row[i]; k < s_row[i + 1]; ++k) {
      const int a = cam_pos[i], c2 = cam_pos[s_col[k]];
      if ((a < 0) != (c2 < 0)) act[(a >= 0 ? a : c2) / B] = 1;
    }
  std::vector<int> &S = pl.sched, elim;
  pl.init_off = 0;
  for (int I = 0; I < pl.p; ++I)
    if (act[I]) S.push_back(I);
  pl.init_cnt = (int)S.size();
  for (int h = 1; h < pl.p; h *= 2) {
    const int fo = (int)S.size();
    for (int I = h; I < pl.p; I += 2 * h)
      if (act[I]) { S.push_back(I); elim.push_back(I); }
    const int uo = (int)S.size();
    for (int J = 0; J < pl.p; J += 2 * h) {
      const bool r = J + h < pl.p && act[J + h], l = J >= h && act[J - h];
      if (!r && !l) continue;
      S.push_back(J | (act[J] ? kUpdHad : 0) | (r ? kUpdRight : 0) | (l ? kUpdLeft : 0));
      act[J] = 1;
    }
    pl.lvl.insert(pl.lvl.end(), {fo, uo - fo, uo, (int)S.size() - uo});
  }
  pl.top_active = act[0] != 0;
  if (pl.top_active) elim.push_back(0);
  pl.elim_off = (int)S.size();
  pl.elim_cnt = (int)elim.size();
  S.insert(S.end(), elim.begin(), elim.end());
  return true;
}

// setup passes (A/B build: SQLM_SCATTER_PF=0 turns the scatter's prefetches off)
#ifndef SQLM_SCATTER_PF
#define SQLM_SCATTER_PF 8
#endif

namespace {

// relaxed atomic min / max (CAS loops, which is what the builtins of the
// compilers that have them expand to on x86)
inline void atomic_min(int *p, int v) {
  int cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
inline void atomic_max(int *p, int v) {
  int cur = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (v > cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

void reset_landmark_stats(const GraphView &g, PlanScratch &ps) {
  fill_par(ps.pt_act, (size_t)g.n_pt, (uint8_t)0);
  fill_par(ps.kcount, (size_t)g.n_pt, 0);
  fill_par(ps.span_lo, (size_t)g.n_pt, std::numeric_limits<int>::max());
  fill_par(ps.span_hi, (size_t)g.n_pt, -1);
  fill_par(ps.efirst, (size_t)g.n_pt, std::numeric_limits<int>::max());
  fill_par(ps.elast, (size_t)g.n_pt, -1);
}

// Active set, track lengths and camera spans in one pass on host threads.
// Fast pass: the chunks start at landmark changes, and a landmark's edges
// are one run (g2o adds a point's edges together, g2oOptimizer.cc:213-281),
// so a run's results are stored plainly; one atomic exchange per run on
// pt_act finds a landmark met twice (false: redo the pass with !fast, relaxed
// atomics for every field). Adds the active edges to n_ae.
bool active_pass(const GraphView &g, PlanScratch &ps, bool fast, int64_t &n_ae) {
  std::vector<uint8_t> &pose_act = ps.pose_act, &pt_act = ps.pt_act;
  std::vector<int> &kcount = ps.kcount, &span_lo = ps.span_lo, &span_hi = ps.span_hi;
  std::vector<int> &efirst = ps.efirst, &elast = ps.elast;
  const int nth = host_threads(g.n_obs);
  std::vector<int64_t> cnt(nth, 0), cut(nth + 1, g.n_obs);
  std::vector<uint8_t> dup(nth, 0);
  for (int t = 0; t < nth; ++t) {  // chunk starts moved forward to a change of landmark
    int64_t e = g.n_obs * t / nth;
    if (fast && t > 0)
      while (e < g.n_obs && e > 0 && g.obs_pt[e] == g.obs_pt[e - 1]) ++e;
    cut[t] = std::max(e, t > 0 ? cut[t - 1] : (int64_t)0);
  }
  run_threads(nth, [&](int t) {
    const int64_t e0 = cut[t], e1 = cut[t + 1];
    int64_t n = 0;
    bool seen_twice = false;
    // runs of one landmark (the reference adds a point's edges together,
    // g2oOptimizer.cc:213-281) are folded locally: one set of atomics per run
    int rl = -1, rk = 0, rlo = 0, rhi = 0, rf = 0, rla = 0;
    auto flush = [&] {
      if (rl < 0) return;
      if (fast && nth > 1) {  // the landmark's only run (checked): plain stores
        seen_twice |= __atomic_exchange_n(&pt_act[rl], (uint8_t)1, __ATOMIC_RELAXED) != 0;
        // (relaxed atomic stores are the same mov; a landmark met by two threads
        // races here until the pass is redone, which plain stores may not)
        __atomic_store_n(&kcount[rl], rk, __ATOMIC_RELAXED);
        __atomic_store_n(&span_lo[rl], rlo, __ATOMIC_RELAXED);
        __atomic_store_n(&span_hi[rl], rhi, __ATOMIC_RELAXED);
        __atomic_store_n(&efirst[rl], rf, __ATOMIC_RELAXED);
        __atomic_store_n(&elast[rl], rla, __ATOMIC_RELAXED);
        return;
      }
      if (nth == 1) {  // one thread (a local-BA window): plain updates (the min / max atomics are CAS loops)
        pt_act[rl] = 1;
        kcount[rl] += rk;
        span_lo[rl] = std::min(span_lo[rl], rlo);
        span_hi[rl] = std::max(span_hi[rl], rhi);
        efirst[rl] = std::min(efirst[rl], rf);
        elast[rl] = std::max(elast[rl], rla);
        return;
      }
      __atomic_store_n(&pt_act[rl], (uint8_t)1, __ATOMIC_RELAXED);
      __atomic_fetch_add(&kcount[rl], rk, __ATOMIC_RELAXED);
      atomic_min(&span_lo[rl], rlo);
      atomic_max(&span_hi[rl], rhi);
      atomic_min(&efirst[rl], rf);
      atomic_max(&elast[rl], rla);
    };
    for (int64_t e = e0; e < e1; ++e) {
      if (g.obs_level[e] != g.level) continue;
      const int l = g.obs_pt[e], pp = g.obs_pose[e];
      if (!__atomic_load_n(&pose_act[pp], __ATOMIC_RELAXED)) __atomic_store_n(&pose_act[pp], (uint8_t)1, __ATOMIC_RELAXED);
      if (l != rl) {
        flush();
        rl = l;
        rk = 0;
        rlo = rhi = pp;
        rf = (int)e;
      }
      ++rk;
      rla = (int)e;
      rlo = std::min(rlo, pp);
      rhi = std::max(rhi, pp);
      ++n;
    }
    flush();
    cnt[t] = n;
    dup[t] = seen_twice;
  });
  if (std::find(dup.begin(), dup.end(), 1) != dup.end()) return false;
  for (int64_t v : cnt) n_ae += v;
  return true;
}

// Landmark slots: bucket by segment width; inside a bucket by camera span
// (first, last observing pose, then id), so a batch of consecutive slots in
// the RCS tiles shares nearly one span (dense MFMA panels).
// (segment width, first pose) buckets by a counting sort, then last pose
// inside a bucket; ties keep id order (the order a stable sort would give)
void sort_landmark_slots(const GraphView &g, PlanScratch &ps, std::vector<int> &pts) {
  const std::vector<uint8_t> &pt_act = ps.pt_act;
  const std::vector<int> &kcount = ps.kcount, &span_lo = ps.span_lo, &span_hi = ps.span_hi;
  auto wl = [](int k) { int w = seg_width(k), b = 0; while ((2 << b) < w) ++b; return b; };  // log2(W) - 1
  const int64_t nb = 7 * (int64_t)g.n_pose + 1;
  std::vector<int> bcnt(nb + 1, 0);
  std::vector<int> &key = ps.key;
  key.resize(g.n_pt);
  // the counting sort on host threads: chunk t (ids in order) histograms its
  // keys, bucket-major / chunk-minor bases keep id order inside a bucket
  const int nk = host_threads(g.n_pt);
  std::vector<std::vector<int>> hist(nk);
  run_threads(nk, [&](int t) {
    std::vector<int> &h = hist[t];
    h.assign(nb, 0);
    for (int l = (int)((int64_t)g.n_pt * t / nk); l < (int)((int64_t)g.n_pt * (t + 1) / nk); ++l) {
      key[l] = pt_act[l] ? (int)(wl(kcount[l]) * (int64_t)g.n_pose + span_lo[l]) : -1;
      if (key[l] >= 0) ++h[key[l]];
    }
  });
  // bucket totals over the chunks, the bucket bases, then every chunk's base
  // inside each bucket (bucket ranges on host threads; one serial pass over
  // nb instead of nb x chunks)
  {
    std::vector<int> &btot = ps.btot;
    btot.resize(nb);
    run_threads(nk, [&](int t) {
      for (int64_t b = nb * t / nk; b < nb * (t + 1) / nk; ++b) {
        int k = 0;
        for (int u = 0; u < nk; ++u) k += hist[u][b];
        btot[b] = k;
      }
    });
    int64_t run = 0;
    for (int64_t b = 0; b < nb; ++b) {
      bcnt[b] = (int)run;
      run += btot[b];
    }
    bcnt[nb] = (int)run;
    run_threads(nk, [&](int t) {
      for (int64_t b = nb * t / nk; b < nb * (t + 1) / nk; ++b) {
        int r = bcnt[b];
        for (int u = 0; u < nk; ++u) { const int k = hist[u][b]; hist[u][b] = r; r += k; }
      }
    });
  }
  pts.resize(bcnt[nb]);
  run_threads(nk, [&](int t) {
    std::vector<int> &f = hist[t];
    for (int l = (int)((int64_t)g.n_pt * t / nk); l < (int)((int64_t)g.n_pt * (t + 1) / nk); ++l)
      if (key[l] >= 0) pts[f[key[l]]++] = l;
  });
  // buckets hold a few dozen points: a stable insertion sort, buckets on host threads
  const int nth = host_threads(g.n_pt * 8);
  run_threads(nth, [&](int t) {
    for (int64_t b = nb * t / nth; b < nb * (t + 1) / nth; ++b) {
      int *v = pts.data() + bcnt[b];
      const int m = bcnt[b + 1] - bcnt[b];
      if (m > 64) {
        std::stable_sort(v, v + m, [&](int a, int bb) { return span_hi[a] < span_hi[bb]; });
        continue;
      }
      for (int i = 1; i < m; ++i) {
        const int x = v[i], key = span_hi[x];
        int j = i - 1;
        while (j >= 0 && span_hi[v[j]] > key) { v[j + 1] = v[j]; --j; }
        v[j + 1] = x;
      }
    }
  });
}

// The slots ascend in segment width (the sort's major key): each bucket ends
// at the first slot of a wider segment.
void make_buckets(const PlanScratch &ps, SetupPlan &pl) {
  const std::vector<int> &pts = pl.slot_pt, &kcount = ps.kcount;
  const int nL = pl.nL;
  pl.buckets.clear();
  pl.upd = UpdLaunch{};
  pl.bucket_part_off.clear();
  pl.n_lm_parts = 0;
  for (int s = 0; s < nL;) {
    const int W = seg_width(kcount[pts[s]]);
    const int e = (int)(std::partition_point(pts.begin() + s, pts.end(), [&](int l) { return seg_width(kcount[l]) <= W; }) -
                        pts.begin());
    // The per-landmark kernels run a bucket with half the lanes its slot-order
    // width names (up to 2 kObsPerLane observations per lane from W = 4 up):
    // longer per-lane Givens chains, fewer idle lanes and butterfly rounds.
    // The slot order -- which the RCS tiles inherit -- stays bucketed at
    // kObsPerLane (config 4: landmark update 0.177 -> 0.160 ms, 775 -> 787
    // it/s, profiles/r05/ab_upd_half_lanes_cr_upd2w.log; the order itself at 4
    // per lane made the tiles 0.05 ms slower, ab_obs_per_lane_rejected.log).
    // (a quarter of the lanes from W = 8 up: 0.160 -> 0.182 ms, ab_uq.log)
    // (one lane per landmark for the shortest tracks: config 4 the same, local
    // BA 7.37k -> 7.22k it/s, ab_upd_one_lane_rejected.log)
    Bucket b{W >= 4 ? W / 2 : W, s, e};
    pl.buckets.push_back(b);
    pl.bucket_part_off.push_back(pl.n_lm_parts);
    pl.n_lm_parts += linearize_blocks(b);
    s = e;
  }
}

// Observations in slot order (edge-id order inside a landmark): offsets by a
// two-pass prefix over slot chunks. False: more than INT_MAX observations.
bool make_lm_begin(const PlanScratch &ps, SetupPlan &pl, int nks) {
  const std::vector<int> &pts = pl.slot_pt, &kcount = ps.kcount;
  const int nL = pl.nL;
  std::vector<int> &lm_begin = pl.lm_begin;
  lm_begin.assign(nL + 1, 0);
  std::vector<int64_t> part(nks + 1, 0);
  run_threads(nks, [&](int t) {
    int64_t acc = 0;
    for (int s = (int)((int64_t)nL * t / nks); s < (int)((int64_t)nL * (t + 1) / nks); ++s) acc += kcount[pts[s]];
    part[t + 1] = acc;
  });
  for (int t = 0; t < nks; ++t) part[t + 1] += part[t];
  if (part[nks] > (int64_t)std::numeric_limits<int>::max()) return false;
  run_threads(nks, [&](int t) {
    int acc = (int)part[t];
    for (int s = (int)((int64_t)nL * t / nks); s < (int)((int64_t)nL * (t + 1) / nks); ++s) {
      acc += kcount[pts[s]];
      lm_begin[s + 1] = acc;
    }
  });
  pl.nE = lm_begin[nL];
  return true;
}

}  // namespace

void plan_active_set(const GraphView &g, bool with_lidar, PlanScratch &ps, SetupPlan &pl, PhaseTimer &phase) {
  ps.pose_act.assign(g.n_pose, 0);
  reset_landmark_stats(g, ps);
  phase("  fills");
  pl.n_ae = 0;
  if (!active_pass(g, ps, true, pl.n_ae)) {  // a landmark in two runs: the atomic pass
    reset_landmark_stats(g, ps);
    active_pass(g, ps, false, pl.n_ae);
  }
  phase("  active pass");
  pl.lid_act.clear();
  if (!with_lidar) return;  // unary pose edges live on rank 0
  for (int64_t e = 0; e < g.n_lid; ++e) {
    if (g.lid_level[e] != g.level || g.pose_fixed[g.lid_pose[e]]) continue;
    pl.lid_act.push_back(e);
    ps.pose_act[g.lid_pose[e]] = 1;
  }
}

int plan_slots(const GraphView &g, PlanScratch &ps, SetupPlan &pl, PhaseTimer &phase) {
  pl.phidx.assign(g.n_pose, -1);
  pl.hidxp.clear();
  for (int p = 0; p < g.n_pose; ++p)
    if (ps.pose_act[p] && !g.pose_fixed[p]) { pl.phidx[p] = (int)pl.hidxp.size(); pl.hidxp.push_back(p); }
  pl.nP = (int)pl.hidxp.size();
  if (pl.nP > kMaxFreePoses) return SQLM_ERR_UNSUPPORTED;
  phase("  lidar+poses");
  std::vector<int> &pts = pl.slot_pt;
  sort_landmark_slots(g, ps, pts);
  const int nL = pl.nL = (int)pts.size();
  phase("active+sort");
  if (pl.nP + nL == 0) return SQLM_ERR_STATE;  // "0 vertices to optimize"
  std::vector<int> &pt_slot = ps.pt_slot;
  fill_par(pt_slot, (size_t)g.n_pt, -1);
  const int nks = host_threads(nL);
  run_threads(nks, [&](int t) {
    for (int s = (int)((int64_t)nL * t / nks); s < (int)((int64_t)nL * (t + 1) / nks); ++s) pt_slot[pts[s]] = s;
  });
  phase("  pt_slot");
  make_buckets(ps, pl);
  if (pl.n_lm_parts > 16384) return SQLM_ERR_UNSUPPORTED;
  phase("  buckets");
  if (!make_lm_begin(ps, pl, nks)) return SQLM_ERR_UNSUPPORTED;
  phase("  lm_begin");
  return SQLM_OK;
}

// Stable scatter of the observations into slot order on a few host threads
// (edge-id order inside a landmark). When every landmark's active edges are
// one contiguous run of edge ids -- g2o's graphs add a point's edges together
// (g2oOptimizer.cc:213-281, 868-912) -- a slot's observations are that run,
// copied front to back. Otherwise chunk t of the edge range counts its edges
// per slot, the per-(chunk, slot) bases follow by a prefix over chunks, then
// every chunk scatters its edges.
void plan_scatter(const GraphView &g, PlanScratch &ps, SetupPlan &pl, const ObsArrays &o, PhaseTimer &phase) {
  const std::vector<int> &pts = pl.slot_pt, &lm_begin = pl.lm_begin, &phidx = pl.phidx;
  const std::vector<int> &kcount = ps.kcount, &efirst = ps.efirst, &elast = ps.elast, &pt_slot = ps.pt_slot;
  const int nL = pl.nL, level = g.level;
  const int nth = host_threads(g.n_obs);
  auto par = [&](auto &&fn) { run_threads(nth, fn); };
  std::vector<uint8_t> inexact(nth, 0);
  // flg: 1 = some input is not a float32 value, 2 = some edge has a robust kernel
  auto put = [&](int64_t e, int ob, int sl, uint8_t &flg) {
    o.dev_edge[ob] = e;
    o.obs_lm[ob] = sl;
    o.obs_cam[ob] = g.obs_pose[e];
    o.obs_camh[ob] = phidx[g.obs_pose[e]];
    const double u = g.obs_uv[2 * e], v = g.obs_uv[2 * e + 1], w = g.obs_info[e], dl = g.obs_delta[e];
    const float fu = (float)u, fv = (float)v, fw = (float)w, fd = (float)dl;
    o.obs_q[4 * (size_t)ob] = fu;
    o.obs_q[4 * (size_t)ob + 1] = fv;
    o.obs_q[4 * (size_t)ob + 2] = fw;
    o.obs_q[4 * (size_t)ob + 3] = fd;
    flg |= ((double)fu != u || (double)fv != v || (double)fw != w || (double)fd != dl) ? 1 : 0;
    flg |= dl > 0.0 ? 2 : 0;
    if (g.obs_ur) o.obs_ur[ob] = g.obs_ur[e];
  };
  bool contig = g.n_obs <= (int64_t)std::numeric_limits<int>::max();
  if (contig) {
    std::vector<uint8_t> split(nth, 0);
    par([&](int t) {
      for (int sl = (int)((int64_t)nL * t / nth); sl < (int)((int64_t)nL * (t + 1) / nth); ++sl) {
        const int l = pts[sl];
        if (elast[l] - efirst[l] + 1 != kcount[l]) { split[t] = 1; break; }
      }
    });
    contig = std::find(split.begin(), split.end(), 1) == split.end();
  }
  phase("  contig check");
  if (contig) {
    // slot order: the outputs are written front to back (whole cache lines)
    // and each landmark's inputs are one run of edge ids
    par([&](int t) {
      uint8_t bad = 0;
      const int s1 = (int)((int64_t)nL * (t + 1) / nth);
      for (int sl = (int)((int64_t)nL * t / nth); sl < s1; ++sl) {
        // the inputs of the landmarks kPf slots ahead (their edge runs sit at
        // random places of the edge arrays), and the run starts 2 kPf ahead
        if (SQLM_SCATTER_PF > 0 && sl + 2 * SQLM_SCATTER_PF < s1) __builtin_prefetch(&efirst[pts[sl + 2 * SQLM_SCATTER_PF]]);
        if (SQLM_SCATTER_PF > 0 && sl + SQLM_SCATTER_PF < s1) {
          const int64_t ep = efirst[pts[sl + SQLM_SCATTER_PF]];
          __builtin_prefetch(&g.obs_uv[2 * ep]);
          __builtin_prefetch(&g.obs_info[ep]);
          __builtin_prefetch(&g.obs_delta[ep]);
          __builtin_prefetch(&g.obs_pose[ep]);
        }
        const int b = lm_begin[sl], k = lm_begin[sl + 1] - b;
        const int64_t e0 = efirst[pts[sl]];
        for (int i = 0; i < k; ++i) put(e0 + i, b + i, sl, bad);
      }
      inexact[t] = bad;
    });
  } else {
    auto ebeg = [&](int t) { return g.n_obs * t / nth; };
    std::vector<std::vector<int>> &base = ps.scat_base;
    if ((int)base.size() < nth) base.resize(nth);
    par([&](int t) {
      std::vector<int> &cnt = base[t];
      cnt.assign(nL, 0);
      for (int64_t e = ebeg(t); e < ebeg(t + 1); ++e)
        if (g.obs_level[e] == level) ++cnt[pt_slot[g.obs_pt[e]]];
    });
    par([&](int t) {  // per-slot prefix over the chunks, slots split across threads
      const int s0 = (int)((int64_t)nL * t / nth), s1 = (int)((int64_t)nL * (t + 1) / nth);
      for (int sl = s0; sl < s1; ++sl) {
        int b = lm_begin[sl];
        for (int u = 0; u < nth; ++u) { const int k = base[u][sl]; base[u][sl] = b; b += k; }
      }
    });
    par([&](int t) {
      std::vector<int> &fill = base[t];
      uint8_t bad = 0;
      for (int64_t e = ebeg(t); e < ebeg(t + 1); ++e) {
        if (g.obs_level[e] != level) continue;
        const int sl = pt_slot[g.obs_pt[e]];
        put(e, fill[sl]++, sl, bad);
      }
      inexact[t] = bad;
    });
  }
  phase("  scatter");
  uint8_t obs_flg = 0;
  for (uint8_t f : inexact) obs_flg |= f;
  pl.obs_f32 = (obs_flg & 1) == 0;
  pl.any_robust = (obs_flg & 2) != 0;
}

// inputs that are not all float32 values: the double arrays, from the same slot order
void plan_scatter_doubles(const GraphView &g, const SetupPlan &pl, const ObsArrays &o) {
  const int nth = host_threads(g.n_obs);
  const int64_t nE = pl.nE;
  run_threads(nth, [&](int t) {
    for (int64_t ob = nE * t / nth; ob < nE * (t + 1) / nth; ++ob) {
      const int64_t ed = o.dev_edge[ob];
      o.obs_uv[2 * ob] = g.obs_uv[2 * ed];
      o.obs_uv[2 * ob + 1] = g.obs_uv[2 * ed + 1];
      o.obs_info[ob] = g.obs_info[ed];
      o.obs_delta[ob] = g.obs_delta[ed];
    }
  });
}

// Camera CSR (device obs in slot order): on the device (launch_cam_csr, after
// the observation upload); on the host, the same chunked counting sort, only
// for a sharded run, whose S pattern union walks it. Otherwise only the count
// of observations seen by a free camera.
void plan_cam_csr(const GraphView &g, bool host_csr, SetupPlan &pl, const ObsArrays &o) {
  const int nP = pl.nP, nth = host_threads(g.n_obs);
  const int64_t nE = pl.nE;
  const int *obs_camh = o.obs_camh;
  auto par = [&](auto &&fn) { run_threads(nth, fn); };
  std::vector<int> &cam_ptr = pl.cam_ptr, &cam_obs = pl.cam_obs;
  cam_ptr.assign(nP + 1, 0);
  cam_obs.clear();
  pl.n_cam_obs = 0;
  if (host_csr) {
    auto obeg = [&](int t) { return nE * t / nth; };
    std::vector<std::vector<int>> base(nth);
    par([&](int t) {
      base[t].assign(nP, 0);
      for (int64_t ob = obeg(t); ob < obeg(t + 1); ++ob)
        if (obs_camh[ob] >= 0) ++base[t][obs_camh[ob]];
    });
    for (int i = 0; i < nP; ++i)
      for (int u = 0; u < nth; ++u) cam_ptr[i + 1] += base[u][i];
    for (int i = 0; i < nP; ++i) cam_ptr[i + 1] += cam_ptr[i];
    for (int i = 0; i < nP; ++i) {
      int b = cam_ptr[i];
      for (int u = 0; u < nth; ++u) { const int k = base[u][i]; base[u][i] = b; b += k; }
    }
    cam_obs.resize(cam_ptr[nP]);
    par([&](int t) {
      std::vector<int> &fill = base[t];
      for (int64_t ob = obeg(t); ob < obeg(t + 1); ++ob)
        if (obs_camh[ob] >= 0) cam_obs[fill[obs_camh[ob]]++] = (int)ob;
    });
    pl.n_cam_obs = (int64_t)cam_obs.size();
  } else {
    std::vector<int64_t> cnt(nth, 0);
    par([&](int t) {
      int64_t k = 0;
      for (int64_t ob = nE * t / nth; ob < nE * (t + 1) / nth; ++ob) k += obs_camh[ob] >= 0;
      cnt[t] = k;
    });
    for (int64_t k : cnt) pl.n_cam_obs += k;
  }
}

// Pose id window of every per-landmark block tile (k_landmark_update): block
// slot ranges in bucket order, then their pose windows on host threads.
void plan_update_windows(const GraphView &g, SetupPlan &pl, const int *obs_cam) {
  const int nth = host_threads(g.n_obs);
  const std::vector<int> &lm_begin = pl.lm_begin;
  std::vector<int2> &upd_rng = pl.upd_rng;
  std::vector<int2> blk_slots;
  for (Bucket &b : pl.buckets) {
    b.rng_off = (int)blk_slots.size();
    const int spb = kBlock / b.W;
    for (int s0 = b.slot_begin; s0 < b.slot_end; s0 += spb) blk_slots.push_back(int2{s0, std::min(s0 + spb, b.slot_end)});
  }
  const size_t nb = blk_slots.size();
  upd_rng.resize(nb);
  run_threads(nth, [&](int t) {
    for (size_t k = nb * t / nth; k < nb * (t + 1) / nth; ++k) {
      int lo = std::numeric_limits<int>::max(), hi = -1;
      for (int ob = lm_begin[blk_slots[k].x]; ob < lm_begin[blk_slots[k].y]; ++ob) {
        lo = std::min(lo, obs_cam[ob]);
        hi = std::max(hi, obs_cam[ob]);
      }
      upd_rng[k] = hi < 0 ? int2{1, 0} : int2{lo, hi};
    }
  });
  for (Bucket &b : pl.buckets) {
    const size_t k1 = b.rng_off + (b.slot_end - b.slot_begin + kBlock / b.W - 1) / (kBlock / b.W);
    b.wide = false;
    for (size_t k = b.rng_off; k < k1 && k < nb; ++k) b.wide |= upd_rng[k].y - upd_rng[k].x + 1 > kUpdWin;
  }
  if (upd_launch_plan(pl.buckets, pl.bucket_part_off, pl.upd)) pl.upd = UpdLaunch{};  // per-bucket launches
}

// Landmarks per tile: up to kTileMaxLm, fewer on small problems so that the
// tiles still cover every CU twice (a local-BA window of 5k landmarks would
// otherwise run ~40 long tiles on 256 CUs)
// (nL / 160, / 80, / 40 measured slower, profiles/r03/ab_lba_tile_lmcap.log)
int tile_lm_cap(int nL) { return std::max(16, std::min(kTileMaxLm, (nL / 512 + 3) & ~3)); }

// A sharded run's local S rows (upper, diagonal first, columns sorted) from
// the host camera CSR. Rows are independent: a few host threads, each with
// its own marks.
void plan_local_rows(const SetupPlan &pl, const ObsArrays &o, std::vector<std::vector<int>> &rows) {
  const int nP = pl.nP;
  const std::vector<int> &cam_ptr = pl.cam_ptr, &cam_obs = pl.cam_obs, &lm_begin = pl.lm_begin;
  rows.assign(nP, {});
  const int nth = host_threads(pl.nE);
  run_threads(nth, [&](int t0) {
    std::vector<int> mark(nP, -1), row;
    for (int i = t0; i < nP; i += nth) {
      row.clear();
      row.push_back(i);
      mark[i] = i;
      for (int t = cam_ptr[i]; t < cam_ptr[i + 1]; ++t) {
        const int s = o.obs_lm[cam_obs[t]];
        for (int ob = lm_begin[s]; ob < lm_begin[s + 1]; ++ob) {
          const int j = o.obs_camh[ob];
          if (j > i && mark[j] != i) { mark[j] = i; row.push_back(j); }
        }
      }
      std::sort(row.begin() + 1, row.end());
      rows[i] = row;
    }
  });
}

void plan_rows_to_pattern(const std::vector<std::vector<int>> &rows, SetupPlan &pl) {
  const int nP = pl.nP;
  std::vector<int> &s_row = pl.s_row, &s_col = pl.s_col;
  s_row.assign(nP + 1, 0);
  for (int i = 0; i < nP; ++i) s_row[i + 1] = s_row[i] + (int)rows[i].size();
  s_col.resize(s_row[nP]);
  for (int i = 0; i < nP; ++i) std::copy(rows[i].begin(), rows[i].end(), s_col.begin() + s_row[i]);
}

void plan_solver(SetupPlan &pl) {
  int mx = 0;
  for (int i = 0; i < pl.nP; ++i) mx = std::max(mx, pl.s_row[i + 1] - pl.s_row[i]);
  pl.max_row_blocks = mx;
  // band (+ border) superblock plan; the dense Cholesky otherwise
  if (!plan_rcs(pl.nP, pl.s_row, pl.s_col, pl.cr, pl.cam_pos)) pl.cr = CRPlan{};
}

void plan_lidar_groups(const GraphView &g, SetupPlan &pl) {
  const int nP = pl.nP;
  std::vector<int> &lid_ptr = pl.lid_ptr, &lid_pose = pl.lid_pose;
  std::vector<double> &lid_data = pl.lid_data;
  lid_ptr.assign(nP + 1, 0);
  lid_pose.clear();
  lid_data.clear();
  std::vector<std::vector<int64_t>> per(nP);
  for (int64_t e : pl.lid_act) per[pl.phidx[g.lid_pose[e]]].push_back(e);
  pl.dev_lid_edge.clear();
  for (int i = 0; i < nP; ++i) {
    lid_ptr[i + 1] = lid_ptr[i] + (int)per[i].size();
    for (int64_t e : per[i]) {
      pl.dev_lid_edge.push_back(e);
      lid_pose.push_back(g.lid_pose[e]);
      for (int k = 0; k < 3; ++k) lid_data.push_back(g.lid_pc[3 * e + k]);
      for (int k = 0; k < 3; ++k) lid_data.push_back(g.lid_pw[3 * e + k]);
      for (int k = 0; k < 3; ++k) lid_data.push_back(g.lid_n[3 * e + k]);
      lid_data.push_back(g.lid_info[e]);
      lid_data.push_back(g.lid_kind && g.lid_kind[e] ? 1.0 : 0.0);  // the edge's kind in the first pad slot
      lid_data.push_back(0.0);
    }
  }
}

}  // namespace sqlm
