#include "spd_solve.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "settings.h"

namespace dpgo {

// The factor stores explicit inverses of the pivot blocks: a pivot range beyond 1e13 (a badly scaled dataset: information
// matrices that differ by many orders of magnitude, or a regulariser far below the weights) leaves few correct digits.
void warn_conditioning(const char *what, const SpdFactor &F) {
  if (F.pivot_min > 0.0 && F.pivot_max / F.pivot_min > 1e13)
    fprintf(stderr, "[dpgo_amd] WARNING: %s is badly conditioned (pivots %.3e .. %.3e, ratio %.1e): expect about %d correct "
                    "digits from its solves.\n", what, F.pivot_min, F.pivot_max, F.pivot_max / F.pivot_min,
            std::max(0, 16 - (int)std::ceil(std::log10(F.pivot_max / F.pivot_min))));
}

struct SpdSolverDev::Plan {
  // one launch.  Tiles [tile0, tile0 + nwide + nnarrow) of the sweep's item list, stored node by node: node a's wide
  // tiles (rows high) are [wstart[a], wstart[a] + wcount[a]), its narrow ones [nstart[a], nstart[a] + ncount[a])
  struct Level {
    int tile0, nwide = 0, nnarrow = 0, rows;
    std::vector<int> wstart, wcount, nstart, ncount;
    std::vector<double> node_bytes;   // algorithmic bytes of the level per node
    Level(int nnodes, int rows, int tile0 = 0)
        : tile0(tile0), rows(rows), wstart(nnodes, 0), wcount(nnodes, 0), nstart(nnodes, 0), ncount(nnodes, 0),
          node_bytes(nnodes, 0.0) {}
    // the launch for the nodes of `bits` (false: none of them has a tile here); bytes: their share of the level
    bool map(NodeBits bits, SpdLevelMap &M, double *bytes = nullptr) const;
  };
  int dof = 1;
  DevBuf<int> piv_idx, upd_idx, asm_ptr, ubuf_dst;
  DevBuf<double> W, WT, ubuf, ytmp;   // W / WT: backward / forward panels (see upload)
  DevBuf<SpdItem> fwd_items, bwd_items;
  DevBuf<PanelSrc> fwd_srcs, bwd_srcs, root_srcs;   // where every tile's panel comes from in the front-major factor
  std::vector<Level> fwd_levels, bwd_levels;   // (without the roots of the trees)
  // the roots: forward and backward step fused into one launch over the explicit inverse of the root's Schur
  // complement (k_spd_level MODE 2); DPGO_SPD_FUSE_ROOT=0 keeps them in the two sweeps
  Level root_level{0, 64};
  bool fused_root = false;
  DevBuf<SpdItem> root_items;
  // the next finer tile class of the full-product roots, for launches over few live roots (upload(), spd_run)
  Level root_fine_level{0, 16};
  DevBuf<SpdItem> root_fine_items;
  DevBuf<double> Wroot_fine;
  int root_fine_rows = 0, root_fine_below = 0;
  // The fused roots stored as ONE TRIANGLE of 64 x 64 blocks (kernels.h: RootRow; k_root_sym + k_root_combine): half the
  // bytes of the level for one small launch more, taken when a single root holds at least DPGO_SPD_ROOT_SYM_MB (32) megabytes
  // (DPGO_SPD_ROOT_SYM=1 / 0 forces it on / off).  root_items are then the wave-sized items, root_sym_level / root_rows_level
  // their and the block rows' per-node ranges, root_part the partial-sum slots, root_pack the per-block descriptors the
  // panels are cut with (also by repack()).
  bool root_sym = false;
  Level root_sym_level{0, 64}, root_rows_level{0, 64};
  DevBuf<RootRow> root_rows;
  DevBuf<double> root_part;
  DevBuf<SpdItem> root_pack;
  DevBuf<double> Wroot, Proot;   // the root tiles' panels; the dense products they are cut from (kept with keep_numeric)
  DevBuf<RootDesc> root_desc;
  int root_max_w = 0;
  SpdDev dev;
  bool stream_once = true;   // panels read with non-temporal loads (see upload)

  // a root of the elimination forest whose forward and backward steps are fused
  bool is_root(const SpdFactor &F, int f) const { return fused_root && F.parent[f] < 0 && F.u[f] == 0 && F.w[f] > 0; }
  const DevBuf<SpdItem> &root_cut() const { return root_sym ? root_pack : root_items; }   // (one triangle: a descriptor per block)
  // Where the dense products P_f = L11^-T L11^-1 of the roots go: root_desc, root_max_w, Proot, p_off[f] (P_f's offset in
  // Proot).  Returns where the roots' W_s = L11^-1 are read from: still on the device after a device factorisation, else
  // uploaded here into `src`.
  const double *stage_roots(const SpdFactor &F, const std::vector<int> &roots, std::vector<int64_t> &p_off, DevBuf<double> &src);
  // Proot <- the products from W_s (launch_root_syrk); Wroot <- the root tiles' panels, cut out of them
  void syrk_and_cut(hipStream_t st, const double *W_s) {
    launch_root_syrk(st, root_desc.p, (int)root_desc.n, root_max_w, W_s, Proot.p);
    launch_pack_panels(st, root_cut().p, root_srcs.p, (int)root_cut().n, Proot.p, Wroot.p);
  }
};

namespace {
// The descriptor of a tile of front f: rows (forward, roots) / pivot columns (backward) first .. first + count; its panel
// starts at mat_off, rows ld doubles apart, entries where spd_panel_index(pair_kq, ...) puts them (spd_panel.h)
SpdItem spd_item(const SpdFactor &F, int f, int first, int count, int ld, int64_t mat_off, int node, int pair_kq = 0) {
  SpdItem it{};
  it.front = f; it.first = first; it.count = count; it.w = F.w[f];
  it.u = F.u[f]; it.ld = ld; it.piv_ptr = F.piv_ptr[f]; it.upd_ptr = F.upd_ptr[f];
  it.pos_off = F.pos_off[f]; it.ubuf_off = F.ubuf_off[f];
  it.node = node; it.mat_off = mat_off; it.pair_kq = pair_kq;
  return it;
}
}  // namespace

SpdItem spd_panel_item(int rows, int count, bool pairs, int64_t mat_off) {
  SpdItem it{};
  it.count = count; it.ld = spd_panel_ld(rows, count); it.pair_kq = spd_pair_kq(pairs, rows); it.mat_off = mat_off;
  return it;
}
int64_t spd_panel_doubles(const SpdItem &it, int64_t len) { return spd_panel_len(it.pair_kq, len) * it.ld; }
void spd_pack_panel_host(const SpdItem &it, const PanelSrc &ps, const double *factor, double *panels) {
  const double *src = factor + ps.src_off;
  double *dst = panels + it.mat_off;
  for (int64_t k = 0; k < ps.len; k++)
    for (int r = 0; r < it.count; r++) dst[spd_panel_index(it.pair_kq, it.ld, k, r)] = src[(size_t)k * ps.src_ld + r];
}

SpdSolverDev::SpdSolverDev() : plan_(new Plan) {}
SpdSolverDev::~SpdSolverDev() { spd_release_device(F); spd_release_numeric(F); }

const double *SpdSolverDev::Plan::stage_roots(const SpdFactor &F, const std::vector<int> &roots, std::vector<int64_t> &p_off,
                                              DevBuf<double> &src) {
  std::vector<double> host_src;
  std::vector<RootDesc> rdesc;
  p_off.assign(F.nfronts, 0);
  int64_t ptotal = 0;
  root_max_w = 0;
  for (int f : roots) {
    RootDesc rd;
    rd.src_off = F.dev_W ? F.w_off[f] : (long long)host_src.size();
    if (!F.dev_W) host_src.insert(host_src.end(), F.W.begin() + F.w_off[f], F.W.begin() + F.w_off[f] + (size_t)F.w[f] * F.ldw[f]);
    rd.dst_off = ptotal; rd.ld = F.ldw[f]; rd.w = F.w[f];
    p_off[f] = ptotal;
    ptotal += (int64_t)F.w[f] * F.w[f];
    root_max_w = std::max(root_max_w, F.w[f]);
    rdesc.push_back(rd);
  }
  root_desc.upload(rdesc);
  Proot.alloc((size_t)ptotal, false);
  if (F.dev_W) return F.dev_W;
  src.upload(host_src);
  return src.p;
}

// Device layout of a factor.  The solve streams every W_s once per sweep, so the matrices are re-packed
// into PANELS: the entries one tile reads, contiguous, in the order it reads them.
//   forward tile (rows p0 .. p0+count of [y ; dupd], all columns k < kend):  panel[k][r] = WT_s[k][p0 + r]
//   backward tile (pivot columns k0 .. k0+count, rows p >= k0):              panel[p - k0][r] = W_s[p][k0 + r]
// (rows of a panel are ld = count rounded up to 16 doubles apart).  The zero triangle of L11^-1 is simply not
// stored, a wave's consecutive loads are consecutive in memory, and every tile is a pure sequential stream.
// With DPGO_SPD_PANEL_PAIRS (the default) the panels of the 64- and 16-row classes hold the two entries a lane consumes
// one after the other side by side (spd_panel.h: panel[k][r] above is entry (k, r) of that map): 16-byte loads.
// Within a launch the tiles are ordered by decreasing length, so the long ones start first and the short
// ones fill the tail.
void SpdSolverDev::upload(int dof, int dcols, const std::vector<int> &node_of_unknown) {
  plan_.reset(new Plan);
  Plan &P = *plan_;
  const Settings &s = settings();
  P.dof = dof;
  P.piv_idx.upload(F.piv_idx);
  P.upd_idx.upload(F.upd_idx);
  P.asm_ptr.upload(F.asm_ptr);
  {
    // pull-ordered update buffer: the a-th entry of the assembly lists is row a; the child row that feeds it
    // (F.asm_src[a]) is told where to write.  Every update row has exactly one reader (its parent).
    std::vector<int> dst(std::max(F.total_upd, 1), 0);
    for (size_t a = 0; a < F.asm_src.size(); a++) dst[F.asm_src[a]] = (int)a;
    P.ubuf_dst.upload(dst);
  }
  P.ubuf.alloc((size_t)std::max(F.total_upd, 1) * dcols);
  P.ytmp.alloc((size_t)std::max(F.n, 1) * dcols);
  // algorithmic bytes of one front: every entry once (8 B) + its in/out vector entries
  // (the pivot block L11^-1 is triangular: w(w+1)/2 entries)
  auto front_bytes = [&](int f) {
    return 8.0 * ((double)F.u[f] * F.w[f] + 0.5 * (double)F.w[f] * (F.w[f] + 1)) + 2.0 * 8.0 * dcols * (F.w[f] + F.u[f]);
  };
  // two classes of tiles: small fronts (one wave per tile) and wide fronts (8 waves per tile, the columns /
  // rows of the reduction split between the waves).
  // The reduction length decides: columns (w) in the forward sweep, rows (w+u) in the backward sweep.
  const int wide_above = 96;   // (<= 128: a narrow tile's reduction is one LDS chunk)
  auto wide = [&](int f, bool fwd) { return (fwd ? F.w[f] : F.w[f] + F.u[f]) > wide_above; };
  // a small narrow class joins the wide class (whole workgroups are cheap when there are few of them)
  auto tiles64 = [&](const std::vector<int> &lvl, bool fwd, bool want_wide) {
    int cnt = 0;
    for (int f : lvl)
      if (wide(f, fwd) == want_wide) cnt += ((fwd ? F.w[f] + F.u[f] : F.w[f]) + 63) / 64;
    return cnt;
  };
  const int MERGE_BELOW = 1024;
  // The roots are applied through the EXPLICIT inverse of their Schur complement (one launch instead of two, below),
  // which is only as good as that complement is conditioned: cancellation costs kappa * eps in every component, where
  // the two triangular sweeps confine the damage to the near-null direction.  So the pivots of every root are looked
  // at first (d_kk = 1 / Linv_kk^2, within the spectrum of the complement), and a factor with a root whose pivots span
  // more than 1e9 -- G_tt of a graph hosted by ONE node is the Laplacian + 1e-11 I, singular along the gauge -- keeps
  // the two sweeps.
  P.fused_root = s.spd_fuse_root;
  // a factor that is re-done every iteration or so (Rescale::Dynamic, G_tt): forming the roots' products again costs 0.5 ms
  // per refactorisation at the headline size, the launch it saves 10 us per solve
  if (F.keep_numeric && !s.spd_fuse_root_dynamic) P.fused_root = false;
  if (P.fused_root) {
    double worst = 1.0;
    std::vector<double> diag;
    for (int f = 0; f < F.nfronts && P.fused_root; f++) {
      if (!P.is_root(F, f)) continue;
      const int w = F.w[f], ld = F.ldw[f];
      diag.assign(w, 0.0);
      if (F.dev_W) HIP_CHECK(hipMemcpy2D(diag.data(), sizeof(double), F.dev_W + F.w_off[f], sizeof(double) * (ld + 1), sizeof(double), w, hipMemcpyDeviceToHost));
      else if (!F.W.empty()) for (int k = 0; k < w; k++) diag[k] = F.W[F.w_off[f] + (size_t)k * ld + k];
      else { P.fused_root = false; break; }
      double lo = 1e300, hi = 0.0;
      for (int k = 0; k < w; k++) { lo = std::min(lo, std::fabs(diag[k])); hi = std::max(hi, std::fabs(diag[k])); }
      if (!(lo > 0.0) || !std::isfinite(hi)) { P.fused_root = false; break; }
      worst = std::max(worst, (hi / lo) * (hi / lo));
    }
    if (worst > std::pow(10.0, s.spd_fuse_root_maxlog)) P.fused_root = false;
    if (s.spd_dump) fprintf(stderr, "[spd] dof %d roots: pivot range %.2e -> %s\n", dof, worst, P.fused_root ? "fused" : "two sweeps");
  }
  std::vector<int> roots;   // the fused roots (none where they stay in the two sweeps)
  for (int f = 0; f < F.nfronts; f++)
    if (P.is_root(F, f)) roots.push_back(f);
  int nnodes = 1;
  for (int a : node_of_unknown) nnodes = std::max(nnodes, a + 1);
  auto node_of_front = [&](int f) { return node_of_unknown[F.piv_idx[F.piv_ptr[f]]]; };   // a front never spans two nodes (they are disconnected)
  struct Tile { int f, first, count; int64_t len; int rows; };   // len: panel rows; rows: tile height of its class (64: also the narrow tiles)
  P.dev.pairs = s.spd_panel_pairs ? 1 : 0;
  auto sweep = [&](bool fwd, std::vector<Plan::Level> &out_levels, DevBuf<SpdItem> &items_dev, DevBuf<double> &panels_dev) {
    const auto &levels = fwd ? F.by_height : F.by_depth;
    std::vector<Tile> tiles;
    out_levels.clear();
    for (const auto &lvl_all : levels) {
      std::vector<int> lvl;   // (the roots have a launch of their own)
      for (int f : lvl_all)
        if (!P.is_root(F, f)) lvl.push_back(f);
      const bool merge = tiles64(lvl, fwd, true) > 0 && tiles64(lvl, fwd, false) < MERGE_BELOW;
      // Few wide tiles at this level: 16-row tiles put 4x more workgroups (CUs) on them.  A workgroup streams
      // ~30-45 GB/s, so a level is as slow as its longest tile whenever it has fewer tiles than the chip has
      // workgroup slots.  Forward tiles re-assemble the front's input vector once per tile, which makes small
      // tiles expensive: 16 rows only below 192 tiles; backward tiles pay off up to 800 tiles when the
      // reduction (front height) is long.  Thresholds from the per-launch table (DPGO_SPD_DUMP) of the
      // headline instance at 8 and at 1 node per GPU.
      const int wide_tiles = tiles64(lvl, fwd, true) + (merge ? tiles64(lvl, fwd, false) : 0);
      int longest = 0;
      for (int f : lvl) longest = std::max(longest, F.w[f] + F.u[f]);
      const bool fine = fwd ? wide_tiles < s.spd_fine_fwd
                            : (wide_tiles < s.spd_fine_bwd || (wide_tiles < s.spd_fine_bwd_tall && longest >= 1000));
      const int rows = (wide_tiles > 0 && fine) ? 16 : 64;
      // node by node; within a node the wide tiles first (one workgroup each, longest first), then the narrow ones
      // (one wave each): a launch picks the ranges of the nodes that are still live (Level::map)
      Plan::Level lev(nnodes, rows, (int)tiles.size());
      for (int f : lvl) lev.node_bytes[node_of_front(f)] += front_bytes(f);
      for (int a = 0; a < nnodes; a++)
        for (int pass = 1; pass >= 0; pass--) {
          const size_t begin = tiles.size();
          const int th = pass == 1 ? rows : 64;
          for (int f : lvl) {
            if (node_of_front(f) != a || (int)(wide(f, fwd) || merge) != pass) continue;
            const int w = F.w[f], m = w + F.u[f], ext = fwd ? m : w;
            for (int r = 0; r < ext; r += th) {
              const int cnt = std::min(th, ext - r);
              // forward: columns k < kend of rows r..; backward: rows p >= r of columns r..
              const int64_t len = fwd ? ((r + th <= w) ? r + th : w) : (m - r);
              tiles.push_back({f, r, cnt, len, th});
            }
          }
          std::stable_sort(tiles.begin() + begin, tiles.end(), [](const Tile &x, const Tile &y) { return x.len * x.count > y.len * y.count; });
          (pass == 1 ? lev.wstart : lev.nstart)[a] = (int)begin;
          (pass == 1 ? lev.wcount : lev.ncount)[a] = (int)(tiles.size() - begin);
          (pass == 1 ? lev.nwide : lev.nnarrow) += (int)(tiles.size() - begin);
        }
      out_levels.push_back(lev);
    }
    // panel offsets, and where every panel's rows are in the front-major factor
    std::vector<SpdItem> items(tiles.size());
    std::vector<PanelSrc> srcs(tiles.size());
    int64_t total = 0;
    for (size_t i = 0; i < tiles.size(); i++) {
      const Tile &t = tiles[i];
      const SpdItem lay = spd_panel_item(t.rows, t.count, P.dev.pairs != 0, total);
      items[i] = spd_item(F, t.f, t.first, t.count, lay.ld, total, node_of_front(t.f), lay.pair_kq);
      if (fwd) srcs[i] = PanelSrc{(long long)(F.wt_off[t.f] + t.first), F.ldm[t.f], (int)t.len};
      else srcs[i] = PanelSrc{(long long)(F.w_off[t.f] + (int64_t)t.first * F.ldw[t.f] + t.first), F.ldw[t.f], (int)t.len};
      total += spd_panel_doubles(items[i], t.len);
    }
    if (s.spd_dump) {
      int64_t used = 0, plain = 0;
      for (const Tile &t : tiles) { used += t.len * t.count; plain += t.len * ((t.count + 15) / 16 * 16); }
      fprintf(stderr, "[spd] dof %d %s panels: %.1f MB stored, %.1f MB of entries (padding %.1f %%, of it %.2f %% whole pad rows of the paired layout), %zu tiles\n",
              dof, fwd ? "fwd" : "bwd", total * 8e-6, used * 8e-6, 100.0 * (total - used) / std::max<int64_t>(used, 1),
              100.0 * (total - plain) / std::max<int64_t>(used, 1), tiles.size());
    }
    items_dev.upload(items);
    if (F.dev_W && F.dev_WT) {
      // the factor is still on the device: the panels are cut out of it there (no trip through the host)
      DevBuf<PanelSrc> &srcs_dev = fwd ? P.fwd_srcs : P.bwd_srcs;   // kept: repack() cuts the panels again after a refactorisation
      srcs_dev.upload(srcs);
      panels_dev.alloc((size_t)std::max<int64_t>(total, 1));   // (zero-filled: the padding of a panel row stays zero)
      launch_pack_panels(nullptr, items_dev.p, srcs_dev.p, (int)tiles.size(), fwd ? F.dev_WT : F.dev_W, panels_dev.p);
      HIP_CHECK(hipDeviceSynchronize());
      return;
    }
    // (what launch_pack_panels does, on the host copy of the factor)
    std::vector<double> panels((size_t)std::max<int64_t>(total, 1), 0.0);
    const double *factor = fwd ? F.WT.data() : F.W.data();
#pragma omp parallel for schedule(dynamic, 16)
    for (size_t i = 0; i < tiles.size(); i++) spd_pack_panel_host(items[i], srcs[i], factor, panels.data());
    panels_dev.upload(panels);
  };
  sweep(true, P.fwd_levels, P.fwd_items, P.WT);
  sweep(false, P.bwd_levels, P.bwd_items, P.W);
  // ---- the roots in the full-product form: tiles of the w x w product L11^-T L11^-1, forward-style (`rows` rows of the
  // front, all columns), node by node; the tiles' items and where their panels are cut from (p_off: stage_roots) into `lev`
  auto root_tiles = [&](int rows, const std::vector<int64_t> &p_off, Plan::Level &lev, std::vector<SpdItem> &items,
                        std::vector<PanelSrc> &srcs) {
    lev = Plan::Level(nnodes, rows);
    int64_t total = 0;
    for (int a = 0; a < nnodes; a++) {
      const size_t begin = items.size();
      for (int f : roots) {
        if (node_of_front(f) != a) continue;
        for (int r = 0; r < F.w[f]; r += rows) {
          const int count = std::min(rows, F.w[f] - r);
          const SpdItem lay = spd_panel_item(rows, count, P.dev.pairs != 0, total);   // (8-row tiles: plain)
          items.push_back(spd_item(F, f, r, count, lay.ld, total, a, lay.pair_kq));
          srcs.push_back(PanelSrc{(long long)(p_off[f] + r), F.w[f], F.w[f]});   // columns r.. of the dense w x w product
          total += spd_panel_doubles(items.back(), F.w[f]);
        }
        lev.node_bytes[a] += 8.0 * (double)F.w[f] * F.w[f] + 2.0 * 8.0 * dcols * F.w[f];
      }
      lev.wstart[a] = (int)begin;
      lev.wcount[a] = (int)(items.size() - begin);
      lev.nwide += (int)(items.size() - begin);
    }
    return total;
  };
  if (!roots.empty()) {
    // one triangle instead of the full product when the roots are big enough for the second (combine) launch to pay
    // (measured, DESIGN 3.4: an item pays three dependent loads for its inputs before 32 KB of stream, and the second
    // launch costs 5 us -- the form wins where ONE root holds tens of megabytes (a single node per GPU: 19.5 -> 15.8 us
    // for G_tt's 44 MB root) and is a wash on eight roots of 8-23 MB each, which keep the full product)
    double largest_mb = 0;
    for (int f : roots) largest_mb = std::max(largest_mb, 8e-6 * (double)F.w[f] * F.w[f]);
    const int force = s.spd_root_sym.value_or(-1);
    P.root_sym = nnodes <= MAX_LOCAL_NODES && (force == 1 || (force != 0 && largest_mb >= s.spd_root_sym_mb));
    std::vector<int64_t> p_off;
    DevBuf<double> src;   // (the roots' W_s, where they had to be uploaded)
    if (P.root_sym) {
      long long nblocks = 0;
      for (int f : roots) { const long long nb = (F.w[f] + 63) / 64; nblocks += nb * (nb + 1) / 2; }
      // blocks per item (a workgroup each, one dependent gather per item): as many as still leave the chip three workgroups
      // per CU, at most ROOT_SYM_MAXJ
      const int S = (int)std::min<long long>(ROOT_SYM_MAXJ, std::max<long long>(1, s.spd_root_sym_blocks.value_or((int)(nblocks / 768))));
      P.root_sym_level = Plan::Level(nnodes, 64);
      P.root_rows_level = P.root_sym_level;
      std::vector<SpdItem> items, pack;
      std::vector<PanelSrc> srcs;
      std::vector<RootRow> rows;
      const double *W_s = P.stage_roots(F, roots, p_off, src);
      int64_t total = 0;
      int nslots = 0;
      for (int a = 0; a < nnodes; a++) {
        P.root_sym_level.nstart[a] = (int)items.size();
        P.root_rows_level.wstart[a] = (int)rows.size();
        for (int f : roots) {
          if (node_of_front(f) != a) continue;
          const int w = F.w[f], nb = (w + 63) / 64;
          const int tbase = nslots;               // transposed slot of block (I, J), J < I: tbase + I (I - 1) / 2 + J
          nslots += nb * (nb - 1) / 2;
          for (int I = 0; I < nb; I++) {
            RootRow rr;
            rr.piv_ptr = F.piv_ptr[f]; rr.first = I * 64; rr.count = std::min(64, w - I * 64); rr.node = a;
            rr.dslot = nslots; rr.ndslots = 0; rr.tbase = tbase; rr.nb = nb; rr.R = I; rr.pad0 = rr.pad1 = rr.pad2 = 0;
            for (int J0 = 0; J0 <= I; J0 += S) {
              const int nJ = std::min(S, I + 1 - J0);
              SpdItem it = spd_item(F, f, I * 64, rr.count, nJ, total, a);
              it.u = J0; it.upd_ptr = nslots++;                     // its direct slot
              it.ubuf_off = tbase + I * (I - 1) / 2 + J0;         // its first transposed slot
              items.push_back(it);
              rr.ndslots++;
              for (int J = J0; J < J0 + nJ; J++) {
                // block (I, J) k-major: row k of the panel = entries (I*64 .. , J*64 + k) of P = row J*64 + k of the symmetric P
                SpdItem pk = it;
                pk.mat_off = total; pk.ld = 64; pk.count = rr.count;
                pack.push_back(pk);
                srcs.push_back(PanelSrc{(long long)(p_off[f] + (int64_t)(J * 64) * w + I * 64), w, std::min(64, w - J * 64)});
                total += 4096;
              }
            }
            rows.push_back(rr);
            P.root_sym_level.node_bytes[a] += 8.0 * 4096.0 * (I + 1);
          }
          P.root_sym_level.node_bytes[a] += 2.0 * 8.0 * dcols * w;
        }
        P.root_sym_level.ncount[a] = (int)items.size() - P.root_sym_level.nstart[a];
        P.root_sym_level.nnarrow += P.root_sym_level.ncount[a];
        P.root_rows_level.wcount[a] = (int)rows.size() - P.root_rows_level.wstart[a];
        P.root_rows_level.nwide += P.root_rows_level.wcount[a];
      }
      P.root_level = P.root_sym_level;   // (what the dumps and the byte counts look at)
      P.root_items.upload(items);
      P.root_pack.upload(pack);
      P.root_srcs.upload(srcs);
      P.root_rows.upload(rows);
      P.root_part.alloc((size_t)std::max(nslots, 1) * 64 * dcols);
      P.Wroot.alloc((size_t)total);   // (zero-filled: rows and columns of a block past w stay zero)
      P.syrk_and_cut(nullptr, W_s);
      if (s.spd_dump)
        fprintf(stderr, "[spd] dof %d fused roots as one triangle: %zu fronts, %zu items of <= %d blocks, %zu block rows, %d slots, %.1f MB of panels\n",
                dof, roots.size(), items.size(), S, rows.size(), nslots, total * 8e-6);
    } else {
      int t64 = 0;
      for (int f : roots) t64 += (F.w[f] + 63) / 64;
      // few tiles: 16-row tiles reach 4x more CUs; a single root per GPU (one node per GPU): 8-row tiles, 8x
      const int rows = t64 < s.spd_fine_root8 ? 8 : (t64 < s.spd_fine_root ? 16 : 64);
      const double *W_s = P.stage_roots(F, roots, p_off, src);
      std::vector<SpdItem> items;
      std::vector<PanelSrc> srcs;
      const int64_t total = root_tiles(rows, p_off, P.root_level, items, srcs);
      P.root_items.upload(items);
      P.root_srcs.upload(srcs);
      P.Wroot.alloc((size_t)total);   // (zero-filled: the padding of a panel row stays zero)
      P.syrk_and_cut(nullptr, W_s);
      // The tile height above fits ALL roots of the group.  The late steps of the truncated CG run on one to four of the
      // group's nodes: a launch over so few roots gets the next finer class (64 -> 16, 16 -> 8 rows: four / two times the
      // workgroups on the same bytes), cut from the same products -- spd_run picks by the number of live tiles.  Not for
      // a factor that is re-done (its panels would have to be cut twice) nor for the fp32 experiment.
      const int fine = rows == 64 ? 16 : (rows == 16 ? 8 : 0);
      if (fine && nnodes > 1 && !F.keep_numeric) {
        std::vector<SpdItem> fitems;
        std::vector<PanelSrc> fsrcs;
        DevBuf<PanelSrc> fsrcs_dev;
        P.Wroot_fine.alloc((size_t)root_tiles(fine, p_off, P.root_fine_level, fitems, fsrcs));
        P.root_fine_items.upload(fitems);
        fsrcs_dev.upload(fsrcs);
        launch_pack_panels(nullptr, P.root_fine_items.p, fsrcs_dev.p, (int)fitems.size(), P.Proot.p, P.Wroot_fine.p);
        HIP_CHECK(hipDeviceSynchronize());
        P.root_fine_rows = fine;
        // (live tiles of the coarse class below which the fine one is taken: the thresholds the class itself was chosen by)
        P.root_fine_below = rows == 64 ? s.spd_fine_root : s.spd_fine_root8;
      }
      if (s.spd_dump)
        fprintf(stderr, "[spd] dof %d fused roots: %zu fronts, %zu tiles x %d rows, %.1f MB of panels\n", dof, roots.size(), items.size(), rows, total * 8e-6);
    }
    HIP_CHECK(hipDeviceSynchronize());
    if (!F.keep_numeric) P.Proot.release();   // (kept for repack() when the factor is re-done with new values)
  }
  spd_release_device(F);
  // the panels are on the device now: the host copy of the factor (gigabytes at the headline size) can go
  std::vector<double>().swap(F.W);
  std::vector<double>().swap(F.WT);
  // both panel sets of a factor this small can live in the 256 MiB Infinity Cache from one solve to the next
  // (measured: G_tt with 177 MB of panels at two nodes per GPU still gains 2 % from staying; 288 MB does not)
  P.stream_once = sizeof(double) * (P.W.n + P.WT.n + P.Wroot.n) > ((size_t)s.spd_keep_mb << 20);
  SpdDev &dev = P.dev;
  dev.piv_idx = P.piv_idx.p; dev.upd_idx = P.upd_idx.p; dev.asm_ptr = P.asm_ptr.p; dev.ubuf_dst = P.ubuf_dst.p;
  dev.W = P.W.p; dev.WT = P.WT.p; dev.fwd_items = P.fwd_items.p; dev.bwd_items = P.bwd_items.p; dev.ubuf = P.ubuf.p;
  dev.root_items = P.root_items.p; dev.Wroot = P.Wroot.p;
}

// New values in the same factor (F.dev_W / F.dev_WT after spd_refactor_device): the panels of every tile are cut out
// again on the device, with the tile lists and sources the first upload() left there.  Enqueued on `st`.
int SpdSolverDev::repack(hipStream_t st) {
  Plan &P = *plan_;
  if (!F.dev_W || !F.dev_WT || P.fwd_srcs.n != P.fwd_items.n || P.bwd_srcs.n != P.bwd_items.n) return -1;
  launch_pack_panels(st, P.fwd_items.p, P.fwd_srcs.p, (int)P.fwd_items.n, F.dev_WT, P.WT.p);
  launch_pack_panels(st, P.bwd_items.p, P.bwd_srcs.p, (int)P.bwd_items.n, F.dev_W, P.W.p);
  if (P.fused_root && P.root_items.n > 0) {
    if (P.root_srcs.n != P.root_cut().n || P.Proot.n == 0) return -1;
    P.syrk_and_cut(st, F.dev_W);
  }
  return 0;
}

bool SpdSolverDev::Plan::Level::map(NodeBits bits, SpdLevelMap &M, double *bytes) const {
  const int nw = spd_waves(rows);
  M.nlive = 0;
  M.pad = tile0;
  int maxw = 0, maxn = 0;
  double b = 0;
  for (int a = 0; a < (int)wcount.size() && a < MAX_LOCAL_NODES; a++) {
    if (!((bits >> a) & 1ull) || wcount[a] + ncount[a] == 0) continue;
    const int j = M.nlive++;
    M.node[j] = (unsigned char)a;
    M.wstart[j] = wstart[a]; M.wcount[j] = wcount[a];
    M.nstart[j] = nstart[a]; M.ncount[j] = ncount[a];
    maxw = std::max(maxw, wcount[a]);
    maxn = std::max(maxn, ncount[a]);
    b += node_bytes[a];
  }
  M.wide_wgs = M.nlive * maxw;
  M.narrow_wgs = M.nlive * ((maxn + nw - 1) / nw);
  if (bytes) *bytes = b;
  return M.nlive > 0;
}

// The tile class of the fused roots for a launch over the nodes `v`: the finer one where few roots are live.  The two classes
// split a row's sum differently (their results differ in the last bits), so the choice must be a function of what the
// ALGORITHM knows -- the nodes live after the last step the host has read (tnt.cpp: live_after) -- never of the launch's
// geometry: a captured CG step, whose launches cover every node, asks with the eager step's node set (class_of below).
bool SpdSolverDev::fine_root_for(NodeBits v) const {
  const Plan &P = *plan_;
  if (P.root_sym || !P.root_fine_rows) return false;
  SpdLevelMap rm;
  if (!P.root_level.map(v, rm)) return false;
  int live_tiles = 0;
  for (int j = 0; j < rm.nlive; j++) live_tiles += rm.wcount[j];
  return live_tiles * P.root_level.rows / 64 < P.root_fine_below;
}

SpdPlanInfo SpdSolverDev::plan_info() const {
  const Plan &P = *plan_;
  auto level = [](const Plan::Level &v) {
    SpdPlanInfo::Level o;
    o.rows = v.rows; o.nwide = v.nwide; o.nnarrow = v.nnarrow; o.wcount = v.wcount; o.ncount = v.ncount;
    return o;
  };
  SpdPlanInfo I;
  I.fused_root = P.fused_root; I.root_sym = P.root_sym; I.stream_once = P.stream_once;
  I.dof = P.dof; I.root_fine_rows = P.root_fine_rows; I.root_fine_below = P.root_fine_below;
  for (const auto &v : P.fwd_levels) I.fwd.push_back(level(v));
  for (const auto &v : P.bwd_levels) I.bwd.push_back(level(v));
  I.root = level(P.root_level);
  I.root_fine = level(P.root_fine_level);
  I.root_rows = level(P.root_rows_level);
  I.nnodes = (int)(I.fwd.empty() ? P.root_level.wcount.size() : I.fwd[0].wcount.size());
  return I;
}

// out <- scale * A^-1 in (the unknowns' entries of the records; everything else in `out` is left alone).
// The forward sweep only reads `in`, the backward sweep only touches `out`: in == out solves in place.
void spd_run(int d, hipStream_t st, SpdSolverDev &S, NodeMask mask, double *in, double *out, double scale, const NodeBits *class_of) {
  const SpdSolverDev::Plan &P = *S.plan_;
  // the launches of the nodes in mask.v (what the host knows); mask.p, if any, is the device's more recent word
  std::vector<SpdLevelMap> fm(P.fwd_levels.size()), bm(P.bwd_levels.size());
  std::vector<double> fby(fm.size(), 0.0), bby(bm.size(), 0.0);
  std::vector<char> fon(fm.size(), 0), bon(bm.size(), 0);
  double bf = 0, bb = 0;
  int nf = 0, nb = 0;
  for (size_t l = 0; l < fm.size(); l++)
    if ((fon[l] = P.fwd_levels[l].map(mask.v, fm[l], &fby[l]))) { bf += fby[l]; nf++; }
  for (size_t l = 0; l < bm.size(); l++)
    if ((bon[l] = P.bwd_levels[l].map(mask.v, bm[l], &bby[l]))) { bb += bby[l]; nb++; }
  SpdLevelMap rm, rrm;
  double rby = 0;
  bool ron = P.root_sym ? (P.root_sym_level.map(mask.v, rm, &rby) && P.root_rows_level.map(mask.v, rrm)) : P.root_level.map(mask.v, rm, &rby);
  // few live roots: the finer tile class (upload()), counted in 64-row tiles as the classes are chosen
  bool fine_root = false;
  if (ron && S.fine_root_for(class_of ? *class_of : mask.v)) {
    fine_root = P.root_fine_level.map(mask.v, rm, &rby);
    ron = fine_root;
  }
  if (ron && in == out) throw DeviceError("spd_run: the fused root step cannot solve in place");
  {
  ProfSweep sweep(true, st, bf + rby, nf + (ron ? (P.root_sym ? 2 : 1) : 0));
  for (size_t l = 0; l < fm.size(); l++)
    if (fon[l]) launch_spd_level(d, P.dof, st, P.dev, 0, fm[l], P.fwd_levels[l].rows, in, P.ytmp.p, scale, fby[l], P.stream_once, mask);
  // the roots: right-hand side from `in` (+ the children's updates), solution straight into `out`
  if (ron && P.root_sym) {
    launch_root_sym(d, P.dof, st, P.dev, rm, in, P.root_part.p, rby, P.stream_once, mask);
    launch_root_combine(d, P.dof, st, P.dev, rrm, P.root_rows.p, P.root_part.p, scale, out, mask);
  } else if (ron && fine_root) {
    SpdDev dv = P.dev;
    dv.root_items = P.root_fine_items.p;
    dv.Wroot = P.Wroot_fine.p;
    launch_spd_level(d, P.dof, st, dv, 2, rm, P.root_fine_rows, in, out, scale, rby, P.stream_once, mask);
  } else if (ron) launch_spd_level(d, P.dof, st, P.dev, 2, rm, P.root_level.rows, in, out, scale, rby, P.stream_once, mask);
  }
  ProfSweep sweep(false, st, bb, nb);
  for (size_t l = 0; l < bm.size(); l++)
    if (bon[l]) launch_spd_level(d, P.dof, st, P.dev, 1, bm[l], P.bwd_levels[l].rows, out, P.ytmp.p, scale, bby[l], P.stream_once, mask);
}

// DPGO_SPD_DUMP=1: time every launch of one solve on a zero vector (HIP events, best of 5) and print its
// algorithmic bytes and rate -- the per-level view behind bench.py's per-family roofline numbers.
void spd_profile(int d, hipStream_t st, SpdSolverDev &S, double *vec) {
  const SpdFactor &F = S.F;
  const SpdSolverDev::Plan &P = *S.plan_;
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  double tot_us = 0, tot_mb = 0;
  unsigned long long *trace = nullptr;
  if (settings().spd_trace) {
    size_t most = 1;
    for (const auto &v : P.fwd_levels) most = std::max(most, (size_t)(v.nwide + v.nnarrow));
    for (const auto &v : P.bwd_levels) most = std::max(most, (size_t)(v.nwide + v.nnarrow));
    most = std::max(most, (size_t)P.root_level.nwide);
    HIP_CHECK(hipMalloc(&trace, most * 6 * 8));
    HIP_CHECK(hipMemset(trace, 0, most * 6 * 8));
    spd_trace_set(trace);
  }
  auto run = [&](int mode, size_t l, const SpdSolverDev::Plan::Level &v, const std::vector<int> &fronts_all) {
    if (v.nwide + v.nnarrow == 0) return;
    const bool fwd = mode != 1;
    int wmax = 0, mmax = 0;
    std::vector<int> fronts;
    for (int f : fronts_all)
      if (P.is_root(F, f) == (mode == 2)) fronts.push_back(f);
    for (int f : fronts) { wmax = std::max(wmax, F.w[f]); mmax = std::max(mmax, F.w[f] + F.u[f]); }
    double bytes = 0;
    for (double b : v.node_bytes) bytes += b;
    float best = 1e30f;
    for (int rep = 0; rep < 6; rep++) {
      HIP_CHECK(hipEventRecord(e0, st));
      SpdLevelMap M;
      v.map(~0ull, M);
      // (mode 2 on a zero vector: in and out may be the same array here, nothing is compared)
      if (mode == 2 && P.root_sym) {
        SpdLevelMap R;
        P.root_rows_level.map(~0ull, R);
        launch_root_sym(d, P.dof, st, P.dev, M, vec, P.root_part.p, 0.0, P.stream_once, ALL_NODES);
        launch_root_combine(d, P.dof, st, P.dev, R, P.root_rows.p, P.root_part.p, 1.0, vec, ALL_NODES);
      } else
      launch_spd_level(d, P.dof, st, P.dev, mode, M, v.rows, vec, mode == 2 ? vec : P.ytmp.p, 1.0, 0.0, P.stream_once, ALL_NODES);
      HIP_CHECK(hipEventRecord(e1, st));
      HIP_CHECK(hipEventSynchronize(e1));
      float ms;
      HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
      if (rep > 0) best = std::min(best, ms);
    }
    tot_us += best * 1e3;
    tot_mb += bytes / 1e6;
    if (trace) {   // (-DSPD_TRACE builds) phase timestamps of the last repetition, 100 MHz ticks -> us
      const int nt = v.nwide + v.nnarrow;
      std::vector<unsigned long long> h((size_t)nt * 6);
      HIP_CHECK(hipMemcpy(h.data(), trace, h.size() * 8, hipMemcpyDeviceToHost));
      unsigned long long tmin = ~0ull;
      for (int t = 0; t < nt; t++) if (h[(size_t)t * 6]) tmin = std::min(tmin, h[(size_t)t * 6]);
      auto pct = [](std::vector<double> &x, double q) { if (x.empty()) return 0.0; std::sort(x.begin(), x.end()); return x[std::min(x.size() - 1, (size_t)(q * x.size()))]; };
      for (int cls = 0; cls < 2; cls++) {
        const int a = cls == 0 ? 0 : v.nwide, b = cls == 0 ? v.nwide : nt;
        if (a == b) continue;
        std::vector<double> ph[5], start, end;
        for (int t = a; t < b; t++) {
          const unsigned long long *q = &h[(size_t)t * 6];
          if (!q[0] || !q[5]) continue;
          for (int i = 0; i < 5; i++) ph[i].push_back((double)(q[i + 1] - q[i]) * 0.01);
          start.push_back((double)(q[0] - tmin) * 0.01);
          end.push_back((double)(q[5] - tmin) * 0.01);
        }
        fprintf(stderr, "[trace]   %s tiles %5zu: item %.2f/%.2f  gather %.2f/%.2f  stream %.2f/%.2f  reduce %.2f/%.2f  write %.2f/%.2f us (median/p90);"
                " start p10 %.1f p50 %.1f p90 %.1f max %.1f, end p10 %.1f p50 %.1f p90 %.1f max %.1f us\n", cls == 0 ? "wide  " : "narrow", start.size(),
                pct(ph[0], .5), pct(ph[0], .9), pct(ph[1], .5), pct(ph[1], .9), pct(ph[2], .5), pct(ph[2], .9), pct(ph[3], .5), pct(ph[3], .9),
                pct(ph[4], .5), pct(ph[4], .9), pct(start, .1), pct(start, .5), pct(start, .9), pct(start, 1.0), pct(end, .1), pct(end, .5),
                pct(end, .9), pct(end, 1.0));
      }
    }
    fprintf(stderr, "[spd] dof %d %s level %2zu fronts %5zu wide tiles %5d x %2d rows, narrow tiles %5d, max_w %4d max_m %4d  %7.2f MB %6.1f us %6.0f GB/s\n",
            P.dof, mode == 2 ? "root" : (fwd ? "fwd" : "bwd"), l, fronts.size(), v.nwide, v.rows, v.nnarrow, wmax, mmax, bytes / 1e6, best * 1e3, bytes / (best * 1e-3) / 1e9);
  };
  std::vector<int> every(F.nfronts);
  for (int f = 0; f < F.nfronts; f++) every[f] = f;
  for (size_t l = 0; l < P.fwd_levels.size(); l++) run(0, l, P.fwd_levels[l], F.by_height[l]);
  run(2, 0, P.root_level, every);
  for (size_t l = 0; l < P.bwd_levels.size(); l++) run(1, l, P.bwd_levels[l], F.by_depth[l]);
  fprintf(stderr, "[spd] dof %d total %.1f MB %.1f us %.0f GB/s (launches timed one by one)\n", P.dof, tot_mb, tot_us, tot_mb / tot_us * 1e3);
  if (trace) {
    spd_trace_set(nullptr);
    HIP_CHECK(hipFree(trace));
  }
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
}

}  // namespace dpgo
