// Sparse SPD direct solver: nested-dissection multifrontal Cholesky.  Separators: minimum vertex covers of BFS-level
// and spectral (Fiedler) cuts, see Dissector in spd.cpp.
//
// Replaces the reference's CHOLMOD factorisations `L_` (of G_tt) and
// `reg_Chol_precon_` (of G_RR + lambda I): C++/DPGO/src/DPGOProblem.cpp:93,119;
// solves at DPGOProblem.h:291, DPGOProblem.cpp:140,568,592.
//
// MI355X-first design: the factorisation happens once on the host (setup, as in
// the reference); what runs per MM iteration is the SOLVE, and a level-scheduled
// sparse triangular solve is latency-poison on a GPU.  So every front s stores
//     W_s = [ L11^-1 ; -L21 L11^-1 ]        ((w+u) x w, dense)
// which turns both sweeps into dense mat-vecs with no triangular dependency
// inside a front:
//     forward :  [y_s ; dupd] = W_s f_s          (f_s = rhs + children's updates)
//     backward:  x_s = W_s^T [y_s ; x_upd]
// Fronts of the same tree height (forward) / depth (backward) are independent and
// run in one launch; each front's update vector is pulled (not pushed) by its
// parent through precomputed gather lists, so the solve is deterministic and
// atomic-free.  W is kept in both orientations so both sweeps read coalesced.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace dpgo {

struct SpdNumericCtx;

struct CsrMatrix {
  int n = 0;
  std::vector<int> ptr, col;
  std::vector<double> val;
};

struct SpdFactorData {
  int n = 0;
  int nfronts = 0;
  std::vector<int> w, u;                 // pivots / update rows per front
  std::vector<int> piv_ptr, piv_idx;     // CSR: matrix indices of the pivots
  std::vector<int> upd_ptr, upd_idx;     // CSR: matrix indices of the update rows
  std::vector<int64_t> w_off, wt_off;    // offset of W_s in W / of WT_s in WT
  std::vector<int> ldw, ldm;             // padded leading dimensions of W_s (>= w) and WT_s (>= w+u)
  int64_t entries = 0;                   // sum (w+u) w: factor entries without padding
  std::vector<double> W;                 // (w+u) x ldw row-major per front
  std::vector<double> WT;                // w x ldm row-major per front
  std::vector<int> parent, height, depth;
  std::vector<int> pos_off;              // first "front position" of each front (w+u positions each)
  std::vector<int> ubuf_off;             // first row of each front's update vector in the update buffer
  std::vector<int> asm_ptr, asm_src;     // per front position: rows of the update buffer to add
  std::vector<std::vector<int>> by_height, by_depth;
  std::vector<std::vector<int>> children;   // elimination tree, kept for spd_refactor
  int total_pos = 0, total_upd = 0, max_front = 0;
  // keep_device: the numeric phase leaves W / WT on the GPU (dev_W / dev_WT, same per-front layout as W / WT, owned by
  // the factor until spd_release_device) and does not fill the host copies -- for callers that only solve on the device
  // smallest / largest pivot d_kk of the factorisation (0 / 0 when not recorded): their ratio is a
  // lower bound of the condition number -- W_s holds the explicit L11^-1, so a huge ratio costs digits in every solve
  double pivot_min = 0.0, pivot_max = 0.0;
  bool keep_device = false;
  // keep_numeric (with keep_device): the device state of the numeric phase stays with the factor (`numeric`), dev_W / dev_WT
  // are borrowed from it, and spd_refactor_device() re-factors from values that are already on the GPU
  bool keep_numeric = false, dev_borrowed = false;
  // quiet: a non-positive pivot is reported by the return value alone, without the ERROR line -- for a caller to whom "not
  // positive definite" is an answer (the certificate's factorisation; the reference: MChol.cholmod().print = 0,
  // C++/SESync/src/SESync_utils.cpp:746-748)
  // factor_only (spd_prepare_device): the numeric phase ends with the verdict and the pivot range -- W / WT are neither
  // allocated nor written, and nothing can be solved with the factor
  bool quiet = false, factor_only = false;
  bool not_pd = false;   // the last numeric phase met a non-positive pivot (a -1 with this unset is a device error)
  int fail_front = -1;   // ... and the front it named (one of them, when several fronts of a level failed); -1 when not_pd is unset
  struct SpdNumericCtx *numeric = nullptr;
  int leaf = 32, collapse = 0, block = 1;   // the parameters this factor was built with (spd_refactor's host path repeats them)
  double *dev_W = nullptr, *dev_WT = nullptr;
  int64_t nnz() const { return entries; }
};
// The factor OWNS `numeric` and (unless borrowed from it) dev_W / dev_WT -- released by spd_release_numeric /
// spd_release_device, which the holder calls -- so a copy would free them twice: factors move, they are never copied.
struct SpdFactor : SpdFactorData {
  SpdFactor() = default;
  SpdFactor(const SpdFactor &) = delete;
  SpdFactor &operator=(const SpdFactor &) = delete;
  SpdFactor(SpdFactor &&o) noexcept : SpdFactorData(std::move(static_cast<SpdFactorData &>(o))) { o.disown(); }
  SpdFactor &operator=(SpdFactor &&o) noexcept {
    if (this != &o) {
      static_cast<SpdFactorData &>(*this) = std::move(static_cast<SpdFactorData &>(o));
      o.disown();
    }
    return *this;
  }

 private:
  void disown() { numeric = nullptr; dev_W = dev_WT = nullptr; dev_borrowed = false; }
};

// Factor A (symmetric positive definite, full pattern in CSR).  leaf = max
// vertices of a nested-dissection leaf.  Returns 0, or -1 if a pivot is not positive.
// collapse = number of nested-dissection levels merged into one front (1 = plain binary tree,
// 0 = choose 1..5 from a latency + bandwidth model of the device solve).
// block > 1: consecutive groups of `block` unknowns share their neighbours (the d rotation rows of a pose); the ordering
// is computed on the quotient graph
int spd_factor(const CsrMatrix &A, SpdFactor &F, int leaf = 32, int collapse = 0, int block = 1, bool keep_device = false);
// frees dev_W / dev_WT (no-op when there are none)
void spd_release_device(SpdFactor &F);

// New values, same pattern (a Dynamic rescale changes the diagonal of G_tt): the numeric phase only, on the GPU
// (spd_dev.hip); without a GPU the whole factorisation is redone.  F must come from spd_factor of the same pattern.
int spd_refactor(const CsrMatrix &A, SpdFactor &F);

// With keep_numeric: the device copy of A's values (CSR order of the matrix that was factored), the numeric phase from
// them, and the release of the kept state (a factor that owns one must not be copied)
double *spd_numeric_values(SpdFactor &F);
// stream (a hipStream_t, nullptr: the factorisation's own): where the kernels run; defer: return as soon as they are
// enqueued -- the caller queues what depends on the new factor behind them on the same stream and calls
// spd_refactor_finish, which waits and returns -1 on a non-positive pivot
int spd_refactor_device(SpdFactor &F, void *stream = nullptr, bool defer = false);
int spd_refactor_finish(SpdFactor &F, bool wait = true);   // wait = false: the stream is known to have passed the factorisation
void spd_release_numeric(SpdFactor &F);

// The three steps of spd_factor taken apart, for a caller that wants to know what a factorisation will cost before it
// allocates anything and whose values are written on the device (the certificate's S + eta I, cert.cpp):
//   spd_symbolic        ordering, fronts, update rows -- from the PATTERN of A alone (A.val is not read; F.quiet and
//                       F.factor_only are kept); F.entries, F.max_front, F.by_height.size() (tree levels) are then known
//   spd_numeric_bytes   the device bytes spd_prepare_device will allocate for that pattern: all front matrices at once,
//                       the value array and the maps into the fronts (+ the padded panels W / WT unless factor_only)
//   spd_prepare_device  the numeric context, kept with the factor (keep_numeric), nothing factored: the caller fills
//                       spd_numeric_values(F) and calls spd_refactor_device.  The context does not depend on any values, so
//                       it survives a factorisation that meets a non-positive pivot: the next call is the kernels again.
int spd_symbolic(const CsrMatrix &A, SpdFactor &F, int leaf, int collapse, int block);
int64_t spd_numeric_bytes(const SpdFactor &F, int64_t nnz);
int spd_prepare_device(const CsrMatrix &A, SpdFactor &F);

// Selected inversion (Takahashi): the entries of A^-1 inside the factor's pattern, front by front, from the explicit
// W_s = [W_top ; W_bot] = [L11^-1 ; -L21 L11^-1].  With S_uu the inverse's block on a front's update rows, taken from its
// parent's finished block through the child -> parent position map of the assembly read the other way:
//     T = S_uu W_bot (u x w),   S_pp = W_top^T W_top + W_bot^T T (w x w),   S_front = [[S_pp, T^T], [T, S_uu]]
// and S_front = W_top^T W_top for a root: dense products, no triangular solve, top-down by tree depth.
// S_front is (w + u) x (w + u) row-major, pivots first, then the update rows, as in W; the fronts lie one after the other
// (spd_selinv_offsets: nfronts + 1 entries).  S_pp is computed for its lower triangle and mirrored, T is stored both ways
// from one product and S_uu is copied from a symmetric block: every S_front is symmetric bit for bit.
//   spd_selinv_host    plain loops over a host copy of W (F.W, or what was read back from dev_W)
//   spd_selinv_bytes   device bytes spd_selinv_device allocates on its first call (the blocks at once, the tile lists)
//   spd_selinv_device  for a factor with keep_device + keep_numeric that is not factor_only, behind a numeric phase that
//                      succeeded (-1, and nothing computed, when the last one met a non-positive pivot); runs on `stream`
//                      (nullptr: the factorisation's own) and returns once it is enqueued.  Fixed summation order, no
//                      atomics: the same bits on every call.  The blocks have storage of their own, so a later
//                      spd_refactor_device gives the bits it gave before.
//   spd_selinv_values  the device blocks (nullptr before the first spd_selinv_device)
//   spd_selinv_release frees them; spd_release_numeric does so too
std::vector<int64_t> spd_selinv_offsets(const SpdFactor &F);
int spd_selinv_host(const SpdFactor &F, const double *W, std::vector<double> &Sigma);
int64_t spd_selinv_bytes(const SpdFactor &F);
int spd_selinv_device(SpdFactor &F, void *stream = nullptr);
const double *spd_selinv_values(const SpdFactor &F);
void spd_selinv_release(SpdFactor &F);

// The device solve for ONE plain vector with the factor as the numeric phase leaves it (dev_W / dev_WT: row-major
// (w + u) x ldw and w x ldm per front, no repacking into SpdSolverDev's panels): x (n doubles, device) <- A^-1 x.
//   forward   one launch per tree height: [y_s ; upd_s] = W_s f_s, f_s the right-hand side on the pivots plus the children's
//             update rows, pulled through per-position lists; y has a buffer of its own
//   backward  one launch per tree depth: x_s = WT_s [y_s ; x(upd_idx)]: reads y and the parents' finished entries of x,
//             writes pivots only
// A workgroup takes 32 rows of one front and stages the front's input vector in LDS (2048 entries at a time); a wave does
// whole rows, lanes striding the row, then a fixed shuffle tree.  No atomics: the same bits on every call.
//   spd_vsolve_bytes    device bytes spd_vsolve_device allocates on its first call (y, the update buffer, the lists)
//   spd_vsolve_device   for a factor with keep_device + keep_numeric that is not factor_only, behind a numeric phase that
//                       succeeded (-1, and nothing computed, otherwise); runs on `stream` (nullptr: the factorisation's own)
//                       and returns once it is enqueued
//   spd_vsolve_release  frees what it allocated; spd_release_numeric does so too
//   spd_vsolve_chunk    how many entries of a front's input vector the launches stage at a time: 1 ... 2048, anything else:
//                       2048, the default and the size of the LDS array; returns the value before.  Process-wide; for the
//                       tests, which want a chunk's edge inside fronts of a few hundred rows.  A multiple of 64 gives the bits
//                       of the default (a lane's terms and their order do not change).
int64_t spd_vsolve_bytes(const SpdFactor &F);
int spd_vsolve_chunk(int chunk);
int spd_vsolve_device(SpdFactor &F, double *x, void *stream = nullptr);
void spd_vsolve_release(SpdFactor &F);

// The device solve for a BLOCK of plain vectors: X (n x k row-major on the device, row length ldx >= k) <- A^-1 X, on dev_W /
// dev_WT as above.  The recursion is spd_vsolve_device's, column block by column block, and with k columns both sweeps are
// products of dense blocks -- (w + u) x w by w x k forward, w x (w + u) by (w + u) x k backward -- on
// v_mfma_f64_16x16x4_f64.  The columns are taken in batches of at most 64, in tiles of 16; a tail batch is padded with zero
// columns that are never stored into X, and the entries X(i, k ... ldx) are not touched.  A workgroup takes 64 rows of one
// front (16 per wave) and stages the front's assembled input block through LDS 32 rows at a time, the next slab's loads in
// flight behind the products.  Y and the update block have buffers of their own (n kb and total_upd kb doubles,
// kb = 16 ceil(min(k, 64) / 16)); the descriptors and the pull lists are spd_vsolve_device's, built by whichever call comes
// first.  No atomics, and no workgroup reads what another of its launch writes: the same bits on every call.  Every output
// entry is ONE sum over the front's depth in ascending order, four terms per instruction, whatever the column: a column's bits
// depend neither on k, nor on its position in a tile or a batch, nor on the other columns.
//   spd_msolve_bytes    device bytes the first spd_msolve_device with batches of kb columns allocates: Y, the update block,
//                       its row items, and spd_vsolve_bytes for the shared lists (counted whether they exist or not)
//   spd_msolve_device   preconditions and return value as spd_vsolve_device (-1, and nothing computed, otherwise; also for
//                       k < 1 or ldx < k); returns once it is enqueued
//   spd_msolve_release  frees what it allocated (not the shared lists: spd_vsolve_release); spd_release_numeric does so too
//   spd_msolve_chunk    how many rows of the assembled input block the launches stage at a time: 1 ... 32, anything else: 32,
//                       the default and the height of the LDS array; returns the value before.  Process-wide; for the tests.
//                       A slab is padded with zero rows to a multiple of four, so a multiple of 4 gives the bits of the
//                       default (every instruction sums the same four terms).
int64_t spd_msolve_bytes(const SpdFactor &F, int kb);
int spd_msolve_chunk(int chunk);
int spd_msolve_device(SpdFactor &F, double *X, int k, int ldx, void *stream = nullptr);
void spd_msolve_release(SpdFactor &F);

// Host solve (setup paths and tests): X (n x ncols, row-major) <- A^-1 X.
void spd_solve_host(const SpdFactor &F, double *X, int ncols);

}  // namespace dpgo
