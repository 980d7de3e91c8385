// The kernels of the Riemannian staircase for gfx950 (stair.h): Lambda and the gradient at a lifted point, the Riemannian
// Hessian, the vector updates of the truncated CG with the preconditioner, the polar retraction, the Gram matrix of the
// rotation rows and the rounding's product with B.
//
// One wave per own segment of the group's SegTable, lane = pose.  A lifted array is two record arrays (columns 0..d-1 and
// d..2d-1); a lane holds its pose's (d+1) x 2d block in registers: every loop over d and 2d is unrolled by the template, no
// local array is indexed at run time.  fp64 throughout, no fast-math.  Every sum is a fixed tree -- lanes of a wave, then the
// segments in order (k_polish_reduce): the same bits run to run, no atomics.
#include "stair.h"

#include "wave_reduce.h"

namespace dpgo {
namespace {

__device__ __forceinline__ bool node_on(const NodeMask &m, int node) { return ((m.p ? (m.v & *m.p) : m.v) >> node) & 1ull; }

// a pose's block of a lifted array: t (2d), then the rows of Y (d x 2d, row-major)
template <int D>
struct LRec {
  double t[2 * D];
  double y[2 * D * D];
};

template <int D>
__device__ __forceinline__ void load_half(const double *p, int row, int off, LRec<D> &o) {
  constexpr int RS = (D + 1) * D;
  const double2 *q = reinterpret_cast<const double2 *>(p + (size_t)row * RS);
  double r[RS];
#pragma unroll
  for (int k = 0; k < RS / 2; k++) {
    const double2 v = q[k];
    r[2 * k] = v.x;
    r[2 * k + 1] = v.y;
  }
#pragma unroll
  for (int c = 0; c < D; c++) o.t[off + c] = r[c];
#pragma unroll
  for (int k = 0; k < D; k++)
#pragma unroll
    for (int c = 0; c < D; c++) o.y[k * 2 * D + off + c] = r[D + k * D + c];
}
template <int D>
__device__ __forceinline__ void load_l(const LiftedC &L, int row, LRec<D> &o) {
  load_half<D>(L.a, row, 0, o);
  load_half<D>(L.b, row, D, o);
}
template <int D>
__device__ __forceinline__ void store_half(double *p, int row, int off, const LRec<D> &o) {
  constexpr int RS = (D + 1) * D;
  double r[RS];
#pragma unroll
  for (int c = 0; c < D; c++) r[c] = o.t[off + c];
#pragma unroll
  for (int k = 0; k < D; k++)
#pragma unroll
    for (int c = 0; c < D; c++) r[D + k * D + c] = o.y[k * 2 * D + off + c];
  double2 *q = reinterpret_cast<double2 *>(p + (size_t)row * RS);
#pragma unroll
  for (int k = 0; k < RS / 2; k++) q[k] = make_double2(r[2 * k], r[2 * k + 1]);
}
template <int D>
__device__ __forceinline__ void store_l(const Lifted &L, int row, const LRec<D> &o) {
  store_half<D>(L.a, row, 0, o);
  store_half<D>(L.b, row, D, o);
}
template <int D>
__device__ __forceinline__ double dot_l(const LRec<D> &a, const LRec<D> &b) {
  double s = 0;
#pragma unroll
  for (int c = 0; c < 2 * D; c++) s = fma(a.t[c], b.t[c], s);
#pragma unroll
  for (int k = 0; k < 2 * D * D; k++) s = fma(a.y[k], b.y[k], s);
  return s;
}
// a += alpha b
template <int D>
__device__ __forceinline__ void axpy_l(double alpha, const LRec<D> &b, LRec<D> &a) {
#pragma unroll
  for (int c = 0; c < 2 * D; c++) a.t[c] = fma(alpha, b.t[c], a.t[c]);
#pragma unroll
  for (int k = 0; k < 2 * D * D; k++) a.y[k] = fma(alpha, b.y[k], a.y[k]);
}

// L = sym(w.Y x.Y^T), d x d row-major
template <int D>
__device__ __forceinline__ void sym_wyT(const LRec<D> &w, const LRec<D> &x, double (&L)[D * D]) {
  double P[D * D];
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < 2 * D; c++) a = fma(w.y[r * 2 * D + c], x.y[s * 2 * D + c], a);
      P[r * D + s] = a;
    }
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) L[r * D + s] = 0.5 * (P[r * D + s] + P[s * D + r]);
}
// w.Y -= L v.Y
template <int D>
__device__ __forceinline__ void sub_Ly(const double (&L)[D * D], const LRec<D> &v, LRec<D> &w) {
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < 2 * D; c++) {
      double a = w.y[r * 2 * D + c];
#pragma unroll
      for (int k = 0; k < D; k++) a = fma(-L[r * D + k], v.y[k * 2 * D + c], a);
      w.y[r * 2 * D + c] = a;
    }
}
// w <- Proj_X(w): w.Y - sym(w.Y x.Y^T) x.Y
template <int D>
__device__ __forceinline__ void proj_l(const LRec<D> &x, LRec<D> &w) {
  double L[D * D];
  sym_wyT<D>(w, x, L);
  sub_Ly<D>(L, x, w);
}
// out = T rec over the d+1 rows [t ; Y], T (d+1) x (d+1) row-major, alike on every column
template <int D>
__device__ __forceinline__ void apply_T(const double *T, const LRec<D> &in, LRec<D> &out) {
  constexpr int B = D + 1;
  double t[B * B];
#pragma unroll
  for (int k = 0; k < B * B; k++) t[k] = T[k];
#pragma unroll
  for (int c = 0; c < 2 * D; c++) {
    double a = t[0] * in.t[c];
#pragma unroll
    for (int j = 0; j < D; j++) a = fma(t[1 + j], in.y[j * 2 * D + c], a);
    out.t[c] = a;
#pragma unroll
    for (int i = 0; i < D; i++) {
      double v = t[(1 + i) * B] * in.t[c];
#pragma unroll
      for (int j = 0; j < D; j++) v = fma(t[(1 + i) * B + 1 + j], in.y[j * 2 * D + c], v);
      out.y[i * 2 * D + c] = v;
    }
  }
}

// one Jacobi rotation of the symmetric 3 x 3 matrix A in the plane (P, Q), accumulated into V (A = V diag V^T at the end)
template <int P, int Q>
__device__ __forceinline__ void jacobi3(double (&A)[9], double (&V)[9]) {
  const double apq = A[P * 3 + Q];
  const double a = A[Q * 3 + Q] - A[P * 3 + P], b = 2.0 * apq;
  const double h = sqrt(fma(a, a, b * b));
  const bool go = h > 1e-300 && apq != 0.0;
  double t = b / (a + (a < 0.0 ? -h : h));
  t = go ? t : 0.0;
  const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double akp = A[k * 3 + P], akq = A[k * 3 + Q];
    A[k * 3 + P] = c * akp - s * akq;
    A[k * 3 + Q] = s * akp + c * akq;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double apk = A[P * 3 + k], aqk = A[Q * 3 + k];
    A[P * 3 + k] = c * apk - s * aqk;
    A[Q * 3 + k] = s * apk + c * aqk;
  }
  A[P * 3 + Q] = 0.0;
  A[Q * 3 + P] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vkp = V[k * 3 + P], vkq = V[k * 3 + Q];
    V[k * 3 + P] = c * vkp - s * vkq;
    V[k * 3 + Q] = s * vkp + c * vkq;
  }
}

// R = C^-1/2 of a symmetric positive definite d x d matrix: d = 2 in closed form (sqrt(C) = (C + s I) / t, s = sqrt(det C),
// t = sqrt(tr C + 2 s)), d = 3 by six cyclic Jacobi sweeps, fully unrolled
template <int D>
__device__ __forceinline__ void inv_sqrt_sym(const double (&C)[D * D], double (&R)[D * D]) {
  if constexpr (D == 2) {
    const double c01 = 0.5 * (C[1] + C[2]);
    const double s = sqrt(fma(C[0], C[3], -(c01 * c01)));
    const double t = sqrt(C[0] + C[3] + 2.0 * s);
    const double inv = 1.0 / (t * s);
    R[0] = (C[3] + s) * inv;
    R[1] = -c01 * inv;
    R[2] = -c01 * inv;
    R[3] = (C[0] + s) * inv;
  } else {
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) A[i * 3 + j] = 0.5 * (C[i * 3 + j] + C[j * 3 + i]);
#pragma unroll
    for (int sweep = 0; sweep < 6; sweep++) {
      jacobi3<0, 1>(A, V);
      jacobi3<0, 2>(A, V);
      jacobi3<1, 2>(A, V);
    }
    const double w0 = 1.0 / sqrt(A[0]), w1 = 1.0 / sqrt(A[4]), w2 = 1.0 / sqrt(A[8]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++)
        R[i * 3 + j] = fma(V[i * 3 + 0] * w0, V[j * 3 + 0], fma(V[i * 3 + 1] * w1, V[j * 3 + 1], V[i * 3 + 2] * w2 * V[j * 3 + 2]));
  }
}

// z.Y = (A A^T)^-1/2 A for A = a.Y, then one Newton-Schulz step Z <- (3/2 I - 1/2 Z Z^T) Z: the eigen-decomposition leaves
// Z Z^T - I of the order u cond(A A^T), the step squares that
template <int D>
__device__ __forceinline__ void polar_l(LRec<D> &a) {
  double C[D * D], R[D * D], z[2 * D * D];
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) {
      double v = 0;
#pragma unroll
      for (int c = 0; c < 2 * D; c++) v = fma(a.y[r * 2 * D + c], a.y[s * 2 * D + c], v);
      C[r * D + s] = v;
    }
  inv_sqrt_sym<D>(C, R);
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < 2 * D; c++) {
      double v = 0;
#pragma unroll
      for (int k = 0; k < D; k++) v = fma(R[r * D + k], a.y[k * 2 * D + c], v);
      z[r * 2 * D + c] = v;
    }
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int s = 0; s < D; s++) {
      double v = 0;
#pragma unroll
      for (int c = 0; c < 2 * D; c++) v = fma(z[r * 2 * D + c], z[s * 2 * D + c], v);
      C[r * D + s] = (r == s ? 1.5 : 0.0) - 0.5 * v;
    }
#pragma unroll
  for (int r = 0; r < D; r++)
#pragma unroll
    for (int c = 0; c < 2 * D; c++) {
      double v = 0;
#pragma unroll
      for (int k = 0; k < D; k++) v = fma(C[r * D + k], z[k * 2 * D + c], v);
      a.y[r * 2 * D + c] = v;
    }
}

#define STAIR_KERNEL_HEAD                    \
  const Seg s = segs[blockIdx.x];            \
  if (!node_on(mask, s.node)) return;        \
  const int row = s.begin + threadIdx.x;     \
  const bool live = row < s.end

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_lambda(const Seg *segs, NodeMask mask, LiftedC X, LiftedC MX,
                                                           double *__restrict__ Lam, Lifted G, double *partial, int nseg) {
  STAIR_KERNEL_HEAD;
  double g2 = 0, F = 0;
  if (live) {
    LRec<D> x, g;
    load_l<D>(X, row, x);
    load_l<D>(MX, row, g);
    F = dot_l<D>(x, g);
    double L[D * D];
    sym_wyT<D>(g, x, L);
#pragma unroll
    for (int k = 0; k < D * D; k++) Lam[(size_t)row * D * D + k] = L[k];
    sub_Ly<D>(L, x, g);
    if (G.a) store_l<D>(G, row, g);
    g2 = dot_l<D>(g, g);
  }
  g2 = wave_sum(g2);
  F = wave_sum(0.5 * F);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = g2;
    partial[(size_t)nseg + blockIdx.x] = F;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_hess(const Seg *segs, NodeMask mask, LiftedC X, const double *__restrict__ Lam,
                                                         LiftedC V, LiftedC MV, Lifted out, double *partial, int nseg) {
  STAIR_KERNEL_HEAD;
  double vw = 0, ww = 0, vv = 0;
  if (live) {
    LRec<D> x, v, w;
    load_l<D>(X, row, x);
    load_l<D>(V, row, v);
    load_l<D>(MV, row, w);
    double L[D * D];
#pragma unroll
    for (int k = 0; k < D * D; k++) L[k] = Lam[(size_t)row * D * D + k];
    sub_Ly<D>(L, v, w);
    proj_l<D>(x, w);
    store_l<D>(out, row, w);
    vw = dot_l<D>(v, w);
    ww = dot_l<D>(w, w);
    vv = dot_l<D>(v, v);
  }
  vw = wave_sum(vw);
  ww = wave_sum(ww);
  vv = wave_sum(vv);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = vw;
    partial[(size_t)nseg + blockIdx.x] = ww;
    partial[(size_t)2 * nseg + blockIdx.x] = vv;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_cg_update(const Seg *segs, NodeMask mask, LiftedC X, const double *__restrict__ Tp,
                                                              int init, int residual, double alpha, LiftedC G, LiftedC P, LiftedC HP,
                                                              Lifted S, Lifted HS, Lifted R, Lifted Z, double *partial, int nseg) {
  STAIR_KERNEL_HEAD;
  double rz = 0, zz = 0;
  if (live) {
    LRec<D> r;
    if (init) {
      LRec<D> zero;
#pragma unroll
      for (int c = 0; c < 2 * D; c++) zero.t[c] = 0.0;
#pragma unroll
      for (int k = 0; k < 2 * D * D; k++) zero.y[k] = 0.0;
      store_l<D>(S, row, zero);
      store_l<D>(HS, row, zero);
      load_l<D>(G, row, r);
    } else {
      LRec<D> a, hp;
      load_l<D>(LiftedC(S), row, a);
      load_l<D>(P, row, hp);
      axpy_l<D>(alpha, hp, a);
      store_l<D>(S, row, a);
      load_l<D>(LiftedC(HS), row, a);
      load_l<D>(HP, row, hp);
      axpy_l<D>(alpha, hp, a);
      store_l<D>(HS, row, a);
      if (residual) {
        load_l<D>(LiftedC(R), row, r);
        axpy_l<D>(alpha, hp, r);
      }
    }
    if (init || residual) {
      store_l<D>(R, row, r);
      LRec<D> z = r;
      if (Tp) {
        LRec<D> x, w = r;
        load_l<D>(X, row, x);
        proj_l<D>(x, w);
        apply_T<D>(Tp + (size_t)row * (D + 1) * (D + 1), w, z);
        proj_l<D>(x, z);
      }
      store_l<D>(Z, row, z);
      rz = dot_l<D>(r, z);
      zz = dot_l<D>(z, z);
    }
  }
  rz = wave_sum(rz);
  zz = wave_sum(zz);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = rz;
    partial[(size_t)nseg + blockIdx.x] = zz;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_cg_dir(const Seg *segs, NodeMask mask, LiftedC Z, double beta, Lifted P) {
  STAIR_KERNEL_HEAD;
  if (live) {
    LRec<D> z, p;
    load_l<D>(Z, row, z);
    load_l<D>(LiftedC(P), row, p);
#pragma unroll
    for (int c = 0; c < 2 * D; c++) p.t[c] = fma(beta, p.t[c], -z.t[c]);
#pragma unroll
    for (int k = 0; k < 2 * D * D; k++) p.y[k] = fma(beta, p.y[k], -z.y[k]);
    store_l<D>(P, row, p);
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_retract(const Seg *segs, NodeMask mask, LiftedC X, LiftedC V, double alpha,
                                                            LiftedC G, LiftedC HV, Lifted Z, double *partial, int nseg) {
  STAIR_KERNEL_HEAD;
  double gv = 0, vv = 0, vhv = 0;
  if (live) {
    LRec<D> x, v;
    load_l<D>(X, row, x);
    load_l<D>(V, row, v);
    vv = dot_l<D>(v, v);
    if (G.a) {
      LRec<D> g;
      load_l<D>(G, row, g);
      gv = dot_l<D>(g, v);
    }
    if (HV.a) {
      LRec<D> h;
      load_l<D>(HV, row, h);
      vhv = dot_l<D>(v, h);
    }
    axpy_l<D>(alpha, v, x);
    polar_l<D>(x);
    store_l<D>(Z, row, x);
  }
  gv = wave_sum(gv);
  vv = wave_sum(vv);
  vhv = wave_sum(vhv);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = gv;
    partial[(size_t)nseg + blockIdx.x] = vv;
    partial[(size_t)2 * nseg + blockIdx.x] = vhv;
  }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_gram(const Seg *segs, NodeMask mask, LiftedC X, double *partial, int nseg) {
  STAIR_KERNEL_HEAD;
  LRec<D> x;
#pragma unroll
  for (int k = 0; k < 2 * D * D; k++) x.y[k] = 0.0;
  if (live) load_l<D>(X, row, x);
  int slot = 0;
#pragma unroll
  for (int a = 0; a < 2 * D; a++)
#pragma unroll
    for (int b = a; b < 2 * D; b++) {
      double v = 0;
#pragma unroll
      for (int k = 0; k < D; k++) v = fma(x.y[k * 2 * D + a], x.y[k * 2 * D + b], v);
      v = wave_sum(v);
      if (threadIdx.x == 0) partial[(size_t)slot * nseg + blockIdx.x] = v;
      slot++;
    }
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_round(const Seg *segs, NodeMask mask, LiftedC X, StairB B, double *__restrict__ W,
                                                          double *partial, int nseg) {
  constexpr int RS = (D + 1) * D;
  STAIR_KERNEL_HEAD;
  double pos = 0;
  if (live) {
    LRec<D> x;
    load_l<D>(X, row, x);
    double w[RS];
#pragma unroll
    for (int j = 0; j < D; j++) {
      double a = 0;
#pragma unroll
      for (int c = 0; c < 2 * D; c++) a = fma(x.t[c], B.v[c * D + j], a);
      w[j] = a;
#pragma unroll
      for (int k = 0; k < D; k++) {
        double v = 0;
#pragma unroll
        for (int c = 0; c < 2 * D; c++) v = fma(x.y[k * 2 * D + c], B.v[c * D + j], v);
        w[D + k * D + j] = v;
      }
    }
    double det;
    if constexpr (D == 2) {
      det = fma(w[2], w[5], -(w[3] * w[4]));
    } else {
      det = w[3] * fma(w[7], w[11], -(w[8] * w[10])) - w[4] * fma(w[6], w[11], -(w[8] * w[9])) + w[5] * fma(w[6], w[10], -(w[7] * w[9]));
    }
    pos = det > 0.0 ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < RS; k++) W[(size_t)row * RS + k] = w[k];
  }
  pos = wave_sum(pos);
  if (threadIdx.x == 0) partial[blockIdx.x] = pos;
}

template <int D>
__global__ __launch_bounds__(SEG_ROWS) void k_stair_copy_t(const Seg *segs, NodeMask mask, const double *__restrict__ W,
                                                           double *__restrict__ out) {
  constexpr int RS = (D + 1) * D;
  STAIR_KERNEL_HEAD;
  if (live) {
#pragma unroll
    for (int c = 0; c < D; c++) out[(size_t)row * RS + c] = W[(size_t)row * RS + c];
  }
}

}  // namespace

#define STAIR_LAUNCH(kernel, ...)                                                                                         \
  do {                                                                                                                    \
    const auto &[d, st, T, mask] = lc;                                                                                    \
    if (T.nseg_own == 0) return;                                                                                          \
    if (d == 3) hipLaunchKernelGGL((kernel<3>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, __VA_ARGS__);      \
    else hipLaunchKernelGGL((kernel<2>), dim3(T.nseg_own), dim3(SEG_ROWS), 0, st, T.segs, mask, __VA_ARGS__);             \
  } while (0)

void launch_stair_lambda(const LaunchCtx &lc, LiftedC X, LiftedC MX, double *Lam, Lifted G, double *partials) {
  STAIR_LAUNCH(k_stair_lambda, X, MX, Lam, G, partials, T.nseg_own);
}
void launch_stair_hess(const LaunchCtx &lc, LiftedC X, const double *Lam, LiftedC V, LiftedC MV, Lifted out, double *partials) {
  STAIR_LAUNCH(k_stair_hess, X, Lam, V, MV, out, partials, T.nseg_own);
}
void launch_stair_cg_update(const LaunchCtx &lc, LiftedC X, const double *Tp, bool init, bool residual, double alpha, LiftedC G,
                            LiftedC p, LiftedC Hp, Lifted s, Lifted hs, Lifted r, Lifted z, double *partials) {
  STAIR_LAUNCH(k_stair_cg_update, X, Tp, init ? 1 : 0, residual ? 1 : 0, alpha, G, p, Hp, s, hs, r, z, partials, T.nseg_own);
}
void launch_stair_cg_dir(const LaunchCtx &lc, LiftedC z, double beta, Lifted p) { STAIR_LAUNCH(k_stair_cg_dir, z, beta, p); }
void launch_stair_retract(const LaunchCtx &lc, LiftedC X, LiftedC V, double alpha, LiftedC G, LiftedC HV, Lifted Z, double *partials) {
  STAIR_LAUNCH(k_stair_retract, X, V, alpha, G, HV, Z, partials, T.nseg_own);
}
void launch_stair_gram(const LaunchCtx &lc, LiftedC X, double *partials) { STAIR_LAUNCH(k_stair_gram, X, partials, T.nseg_own); }
void launch_stair_round(const LaunchCtx &lc, LiftedC X, const StairB &B, double *W, double *partials) {
  STAIR_LAUNCH(k_stair_round, X, B, W, partials, T.nseg_own);
}
void launch_stair_copy_t(const LaunchCtx &lc, const double *W, double *out) { STAIR_LAUNCH(k_stair_copy_t, W, out); }

}  // namespace dpgo
