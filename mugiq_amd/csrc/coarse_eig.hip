// The coarse-grid eigensolver: Chebyshev-filtered block subspace iteration on A = MdagM | MMdag of the explicit coarse operator
// (csrc/coarse_op.hip), what Eigsolve_Mugiq::computeEvecs does on mg_env->diracCoarse in the reference's computeCoarse branch
// (lib/eigsolve_mugiq.cpp:27-33, 278-287).  Contracts: mugiq_hip_coarse_gram, mugiq_hip_coarse_rotate and mugiq_hip_coarse_eigensolve in
// include/mugiq_hip.h; the algorithm, step for step: tests/coarse_eig_ref.py.  fp64 only.  On a process grid
// (mugiq_hip_coarse_gram_grid, mugiq_hip_coarse_eigensolve_grid; tests/coarse_eig_grid_ref.py) the operator exchanges faces
// (coarse_apply_grid), every Gram matrix and every residual sum is added over the ranks (sum_over_ranks), and everything else is local to
// a rank or dense host algebra repeated on identical input; the Chebyshev step writes the send faces of the next application.
//
// A coarse vector is seen as the list of its L = 2 N volumeCB body elements, N = 2 n_vec, in the order (parity, row s n_vec + c, x_cb):
// element e of a padded field sits at parity parity_offset + row stride + x_cb, of a packed one (stride = volumeCB, parity_offset =
// N stride: the solver's work bases) at e.  Both block kernels are complex GEMMs on v_mfma_f64_16x16x4_f64 with the complex structure
// unfolded into real products (the idiom of csrc/momproj.hip and csrc/prolong.hip: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j =
// lane & 15], D[(lane >> 4) + 4 r][lane & 15] in register r); neither uses LDS.
//
// coarse_gram_kernel: G[i][j] = <a_i, b_j>.  The k index of the instruction runs over vector elements: a wave owns a 16 x 16 tile of G
// and walks a chunk of kGramChunk elements eight at a time -- lane (i, k) reads elements 2 k and 2 k + 1 of the eight, so the four lanes
// of a row read one 128-byte line -- with Re G and Im G in one accumulator each, updated in a fixed order (re re, im im | re im, -im re).
// Sums are kept short: 16 elements make one chain (a leaf), the 16 leaves of a run of 256 elements are added in order, the 16 runs of a
// chunk in order, and coarse_gram_sum_kernel adds the chunks eight to a run (a single chain over 4096 positive terms, the diagonal of a
// Gram matrix, was measured 9 eps off, and chains of 256 elements 6.8 eps on short vectors, past the 4 eps sum |a| |b| the tests hold it
// to: gram_walk).
// The partial of a chunk goes to memory, coarse_gram_sum_kernel adds the chunks in ascending order.  The chunk depends on nothing, the
// walk on L alone, and an entry of the tile on its own row and column alone: the bits of G[i][j] are those of (a_i, b_j) in any batch.
//
// coarse_rotate_kernel: out_j = sum_i in_i Z[i][j], computed transposed, D[j][e] = sum_i Z^T[j][i] in_i[e], so that the element stays on the lane and a
// store is 16 consecutive complex numbers.  k runs over the input vectors, four to an instruction, in ascending order; a wave owns 32
// elements x 64 outputs (16 accumulators).  Z comes zero-padded to multiples of (4, 64) behind the pointer table.
#include "mg_common.h"
#include "op_forms.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

namespace mugiq {
// csrc/dense_herm.cpp
int hermitian_eigh(int n, const double *H, double *theta, double *Z, const char *who);
int cholesky_upper(int n, const double *G, double *R, double rankTol, int *badPivot, double *pivot, const char *who);
int upper_inverse(int n, const double *R, double *Rinv, const char *who);

namespace {

constexpr int kEigBlock = 8;         // vectors per call of the batched operator
constexpr int kEigMaxKr = 512;
constexpr int kGramChunk = 4096;     // complex elements of a vector per partial Gram matrix
constexpr int kGramStep = 8;         // ... per trip of a wave
constexpr int kGramLeaf = 16;        // ... summed in one chain before they join the run's sum (divides 32, which divides every vector)
constexpr int kGramRun = 256;        // ... whose leaves are added in one chain before they join the chunk's sum (divides kGramChunk)
constexpr int kGramFan = 8;          // chunks added in one chain by coarse_gram_sum_kernel before they join the total
constexpr int kRotElems = 32;        // rotate: elements per wave,
constexpr int kRotOut = 64;          // ... outputs per wave,
constexpr int kRotWaves = 4;         // ... waves per workgroup
constexpr int kEwThreads = 256;
constexpr int kStepRows = 8;         // rows a thread of chebyshev_step_pack_kernel walks at most from one set of coordinates
constexpr bool kEigPackInStepDefault = true;  // the measurement the default follows
constexpr int kPowerSteps = 20;      // first guess, NOT tuned (QUDA: 100)
constexpr double kAmaxMargin = 1.1;  // QUDA's

typedef Cplx<double> Z;
typedef double d4 __attribute__((ext_vector_type(4)));

// total = 2 rows rowLen = 4 n_vec volumeCB is a multiple of 32 for every field check_fields admits (four even extents: volumeCB is a
// multiple of 8); the kernels rely on it: a wave's 8 (Gram) or 32 (rotation) elements are all there or none is
struct VecGeom {
  int rowLen, rows;  // volumeCB, N
  int stride;
  int packed;
  int64_t po, total;
};
__device__ inline int64_t ce_offset(const VecGeom &g, int64_t e) {
  if (g.packed) return e;
  const int64_t row = e / g.rowLen;
  const int pty = row >= g.rows ? 1 : 0;
  return pty * g.po + (row - pty * g.rows) * (int64_t)g.stride + (e - row * g.rowLen);
}

// ---- Gram ------------------------------------------------------------------------------------------------------------------------------
struct GramArgs {
  const void *const *tab;  // mA bodies of a, then mB bodies of b
  int mA, mB;
  VecGeom ga, gb;
  Z *partial;  // [chunk][mA][mB]
};

__device__ inline void gram_walk(const void *pa, const void *pb, const VecGeom &ga, const VecGeom &gb, int64_t e0, int64_t e1, int k, d4 &re, d4 &im) {
  // three levels: a leaf of kGramLeaf elements is summed on its own (8 instructions, 32 products to an accumulator), the leaves of a run
  // of kGramRun elements are added in order, and the runs in order to the chunk's sum.  The instruction adds its four products one after
  // the other, each sum rounded, so a chain of n elements is a chain of 2 n roundings: on the diagonal of a Gram matrix (all terms
  // positive) a single chain over 4096 elements was measured 9 eps off, and runs of 256 without leaves reached 6.8 eps among the 264
  // diagonal entries of vectors of 320 elements, which have only two runs to average over -- past the 4 eps sum |a| |b| the tests hold
  // the kernel to.  With leaves no level adds more than 32 terms in a row (1.9 eps at most over the shapes of
  // tests/test_coarse_eig_cpu.py, which restates this tree in numpy).
  // L is a multiple of 32 (VecGeom), so the last run of a vector may be short but no leaf and no trip of 8 elements is
  for (int64_t s0 = e0; s0 < e1; s0 += kGramRun) {
    const int64_t s1 = min(s0 + (int64_t)kGramRun, e1);
    d4 rr = {0.0, 0.0, 0.0, 0.0}, ri = {0.0, 0.0, 0.0, 0.0};
    for (int64_t l0 = s0; l0 < s1; l0 += kGramLeaf) {
      d4 lr = {0.0, 0.0, 0.0, 0.0}, li = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int64_t b = l0; b < l0 + kGramLeaf; b += kGramStep) {
        Z x[2], y[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const int64_t e = b + 2 * k + u;
          x[u] = ld_wide<double>(pa, ce_offset(ga, e));
          y[u] = ld_wide<double>(pb, ce_offset(gb, e));
        }
#pragma unroll
        for (int u = 0; u < 2; u++) {
          lr = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].re, y[u].re, lr, 0, 0, 0);
          lr = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].im, y[u].im, lr, 0, 0, 0);
          li = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].re, y[u].im, li, 0, 0, 0);
          li = __builtin_amdgcn_mfma_f64_16x16x4f64(-x[u].im, y[u].re, li, 0, 0, 0);
        }
      }
      rr += lr;
      ri += li;
    }
    re += rr;
    im += ri;
  }
}

// grid (chunks, ceil(mA / 32), ceil(mB / 32)); wave w of the four owns the tile (w >> 1, w & 1) of the 32 x 32 block
__global__ __launch_bounds__(256) void coarse_gram_kernel(GramArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, k = lane >> 4;
  const int i0 = blockIdx.y * 32 + (w >> 1) * 16, j0 = blockIdx.z * 32 + (w & 1) * 16;
  if (i0 >= a.mA || j0 >= a.mB) return;  // the whole wave
  // rows and columns past the end shadow the last vector: a row of the product depends on its own operand row alone
  const void *pa = as_global(a.tab)[min(i0 + r, a.mA - 1)], *pb = as_global(a.tab)[a.mA + min(j0 + r, a.mB - 1)];
  const int64_t e0 = (int64_t)blockIdx.x * kGramChunk, e1 = min(e0 + (int64_t)kGramChunk, a.ga.total);
  d4 re = {0.0, 0.0, 0.0, 0.0}, im = {0.0, 0.0, 0.0, 0.0};
  gram_walk(pa, pb, a.ga, a.gb, e0, e1, k, re, im);
  Z *out = a.partial + (size_t)blockIdx.x * a.mA * a.mB;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int i = i0 + k + 4 * q, j = j0 + r;
    if (i < a.mA && j < a.mB) st_round<double>(out, (int64_t)i * a.mB + j, Z{re[q], im[q]});
  }
}

__global__ __launch_bounds__(256) void coarse_gram_sum_kernel(const Z *partial, int nChunks, int nEntries, Z *G) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nEntries) return;
  // chunks in ascending order, kGramFan to a run, the runs in ascending order
  Z s{0.0, 0.0};
  for (int c0 = 0; c0 < nChunks; c0 += kGramFan) {
    Z run = ld_wide<double>(partial, (int64_t)c0 * nEntries + idx);
    for (int c = c0 + 1; c < min(c0 + kGramFan, nChunks); c++) {
      const Z p = ld_wide<double>(partial, (int64_t)c * nEntries + idx);
      run.re += p.re;
      run.im += p.im;
    }
    s.re += run.re;
    s.im += run.im;
  }
  st_round<double>(G, idx, s);
}

// ---- rotation --------------------------------------------------------------------------------------------------------------------------
struct RotArgs {
  const void *const *tab;  // mIn bodies of in, then mOut bodies of out
  const double *zre, *zim;  // [mInPad][ldz], zero beyond (mIn, mOut)
  int mIn, mOut, mInPad, ldz;
  VecGeom gi, go;
};

// grid (ceil(L / 128), ceil(mOut / 64))
__global__ __launch_bounds__(64 * kRotWaves) void coarse_rotate_kernel(RotArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = lane & 15, k = lane >> 4;
  const int64_t eBase = ((int64_t)blockIdx.x * kRotWaves + w) * kRotElems;
  if (eBase >= a.gi.total) return;  // the whole wave; L is a multiple of kRotElems (VecGeom), so a wave that stays has all its elements
  const int jBase = blockIdx.y * kRotOut;
  constexpr int EB = kRotElems / 16, JB = kRotOut / 16;
  int64_t offIn[EB];
#pragma unroll
  for (int eb = 0; eb < EB; eb++) offIn[eb] = ce_offset(a.gi, eBase + 16 * eb + q);
  d4 accRe[EB][JB], accIm[EB][JB];
#pragma unroll
  for (int eb = 0; eb < EB; eb++)
#pragma unroll
    for (int jb = 0; jb < JB; jb++) accRe[eb][jb] = accIm[eb][jb] = d4{0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < a.mInPad; i0 += 4) {
    const int i = i0 + k;
    const void *p = as_global(a.tab)[min(i, a.mIn - 1)];
    Z x[EB];
#pragma unroll
    for (int eb = 0; eb < EB; eb++) x[eb] = i < a.mIn ? ld_wide<double>(p, offIn[eb]) : Z{0.0, 0.0};
    double zr[JB], zi[JB];
#pragma unroll
    for (int jb = 0; jb < JB; jb++) {
      const int64_t at = (int64_t)i * a.ldz + jBase + 16 * jb + q;
      zr[jb] = *as_global(a.zre + at);
      zi[jb] = *as_global(a.zim + at);
    }
#pragma unroll
    for (int eb = 0; eb < EB; eb++)
#pragma unroll
      for (int jb = 0; jb < JB; jb++) {
        accRe[eb][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr[jb], x[eb].re, accRe[eb][jb], 0, 0, 0);
        accRe[eb][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(-zi[jb], x[eb].im, accRe[eb][jb], 0, 0, 0);
        accIm[eb][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(zi[jb], x[eb].re, accIm[eb][jb], 0, 0, 0);
        accIm[eb][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(zr[jb], x[eb].im, accIm[eb][jb], 0, 0, 0);
      }
  }
#pragma unroll
  for (int eb = 0; eb < EB; eb++) {
    const int64_t off = ce_offset(a.go, eBase + 16 * eb + q);
#pragma unroll
    for (int jb = 0; jb < JB; jb++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int j = jBase + 16 * jb + k + 4 * r;
        if (j < a.mOut) st_round<double>(const_cast<void *>(as_global(a.tab)[a.mIn + j]), off, Z{accRe[eb][jb][r], accIm[eb][jb][r]});
      }
  }
}

// ---- elementwise, on packed vectors `pitch` elements apart (the solver's work memory) -----------------------------------------------------
// out_v = alpha y_v + beta t_v [- prev_v], v < n <= 8: one step of the Chebyshev recurrence.  out may be t or prev
struct ChebArgs {
  Z *out;
  const Z *y, *t, *prev;  // prev NULL: the first step
  int64_t pitch, total;
  double alpha, beta;
};
// element `at` of the step: the one expression of both step kernels, so their values are the same bits by construction
__device__ inline Z chebyshev_value(const ChebArgs &a, int64_t at) {
  const Z y = ld_wide<double>(a.y, at), t = ld_wide<double>(a.t, at);
  Z o{fma(a.alpha, y.re, a.beta * t.re), fma(a.alpha, y.im, a.beta * t.im)};
  if (a.prev) {
    const Z p = ld_wide<double>(a.prev, at);
    o.re -= p.re;
    o.im -= p.im;
  }
  return o;
}
__global__ __launch_bounds__(kEwThreads) void chebyshev_step_kernel(ChebArgs a) {
  const int64_t base = (int64_t)blockIdx.y * a.pitch;
  for (int64_t e = (int64_t)blockIdx.x * kEwThreads + threadIdx.x; e < a.total; e += (int64_t)gridDim.x * kEwThreads)
    st_round<double>(a.out, base + e, chebyshev_value(a, base + e));
}

// The step on a process grid: the same values, and where the site of an element lies on the low or the high face of a partitioned axis
// the element goes to that face's send buffer as well, in the layout of face_pack_kernel (csrc/coarse_op.hip):
// send[mu][high][((v 2 + parity) rows + row) faceCB + f], f = ghost_face_index_on_face.  A site can be on faces of several axes (with
// extent 2 it is on one of the two faces of that axis) and then stores to each; plain vector stores, no atomics, no LDS.
// A thread owns one site (vector v, parity, x_cb) and a subset of its rows: lane = x_cb within a tile of 64, so every load and the body
// store of a wave are 64 consecutive complex numbers of one row; the coordinates and the face indices are worked out once per thread,
// ahead of the rows.  The stores to a face are consecutive in f where the lanes' sites are (the x face: scattered).
// grid (ceil(volumeCB / 64), 2 kEigBlock, row chunks), 4 waves: wave w of chunk z walks the rows 4 z + w, + 4 gridDim.z, ...
struct ChebPackArgs {
  ChebArgs c;
  int X[4], volumeCB, rows;
  int part[4], faceCB[4];
  Z *send[4][2];
};
__global__ __launch_bounds__(kEwThreads) void chebyshev_step_pack_kernel(ChebPackArgs a) {
  const int x_cb = blockIdx.x * 64 + (threadIdx.x & 63), v = blockIdx.y >> 1, par = blockIdx.y & 1;
  if (x_cb >= a.volumeCB) return;
  int c[4];
  get_coords(c, x_cb, a.X, par);
  Z *face[4];
  int64_t fbase[4];
#pragma unroll
  for (int mu = 0; mu < 4; mu++) {
    face[mu] = nullptr;
    fbase[mu] = 0;
    if (!a.part[mu]) continue;
    const int high = c[mu] == a.X[mu] - 1 ? 1 : 0;
    if (!high && c[mu] != 0) continue;
    face[mu] = a.send[mu][high];
    fbase[mu] = (int64_t)blockIdx.y * a.rows * a.faceCB[mu] + ghost_face_index_on_face(c, a.X, mu);
  }
  const int64_t base = (int64_t)v * a.c.pitch + (int64_t)par * a.rows * a.volumeCB + x_cb;
  for (int row = blockIdx.z * (kEwThreads / 64) + (threadIdx.x >> 6); row < a.rows; row += gridDim.z * (kEwThreads / 64)) {
    const int64_t at = base + (int64_t)row * a.volumeCB;
    const Z o = chebyshev_value(a.c, at);
    st_round<double>(a.c.out, at, o);
#pragma unroll
    for (int mu = 0; mu < 4; mu++)
      if (face[mu]) st_round<double>(face[mu], fbase[mu] + (int64_t)row * a.faceCB[mu], o);
  }
}

// partial[v][chunk] = sum over the chunk of |W_v - theta_v Q_v|^2: per lane over its elements in ascending order, down the wave by
// shuffles, the four waves in ascending order; residual_sum_kernel adds the chunks in ascending order.  grid (chunks, vectors)
__global__ __launch_bounds__(kEwThreads) void residual_partial_kernel(const Z *W, const Z *Q, const double *theta, int64_t pitch, int64_t total, double *partial) {
  __shared__ double sh[kEwThreads / 64];
  const int v = blockIdx.y, t = threadIdx.x;
  const double th = theta[v];
  const int64_t base = (int64_t)v * pitch, e0 = (int64_t)blockIdx.x * kGramChunk, e1 = min(e0 + (int64_t)kGramChunk, total);
  double s = 0.0;
  for (int64_t e = e0 + t; e < e1; e += kEwThreads) {
    const Z w = ld_wide<double>(W, base + e), q = ld_wide<double>(Q, base + e);
    const double dr = fma(-th, q.re, w.re), di = fma(-th, q.im, w.im);
    s = fma(dr, dr, s);
    s = fma(di, di, s);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((t & 63) == 0) sh[t >> 6] = s;
  __syncthreads();
  if (t == 0) partial[(size_t)v * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
__global__ __launch_bounds__(kEwThreads) void residual_sum_kernel(const double *partial, int nChunks, int nVec, double *out) {
  const int v = blockIdx.x * kEwThreads + threadIdx.x;
  if (v >= nVec) return;
  double s = 0.0;
  for (int c = 0; c < nChunks; c++) s += partial[(size_t)v * nChunks + c];
  out[v] = s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
VecGeom vec_geom(const MugiqHipCoarseField &f) {
  VecGeom g;
  g.rowLen = f.volumeCB;
  g.rows = 2 * f.nColor;
  g.stride = f.stride;
  g.po = f.parity_offset;
  g.packed = (f.stride == f.volumeCB && f.parity_offset == (int64_t)g.rows * f.stride) ? 1 : 0;
  g.total = (int64_t)2 * g.rows * f.volumeCB;
  return g;
}

// n coarse fields of one geometry, stride and parity offset (that of `like` if given), fp64
int check_fields(const MugiqHipCoarseField *f, int n, const MugiqHipCoarseField *like, const char *who, const char *name) {
  for (int i = 0; i < n; i++) {
    const MugiqHipCoarseField &w = f[i];
    MUGIQ_REQUIRE(w.data != nullptr, "%s: %s vector %d is NULL", who, name, i);
    MUGIQ_REQUIRE(w.precision == 4 || w.precision == 8, "%s: %s vector %d has precision %d", who, name, i, w.precision);
    if (w.precision != 8) return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: %s vector %d has precision %d: the eigensolver's kernels are fp64 only", who, name, i, w.precision);
    MUGIQ_REQUIRE(w.nSpin == 2 && w.nColor >= 1, "%s: %s vector %d has nSpin %d, nColor %d (a coarse field has nSpin 2)", who, name, i, w.nSpin, w.nColor);
    long long vol = 1;
    for (int d = 0; d < 4; d++) {
      MUGIQ_REQUIRE(w.X[d] > 0 && (w.X[d] & 1) == 0, "%s: %s vector %d: X[%d] = %d must be positive and even", who, name, i, d, w.X[d]);
      vol *= w.X[d];
    }
    MUGIQ_REQUIRE(vol / 2 < (1LL << 30) && w.volumeCB == (int)(vol / 2), "%s: %s vector %d: volumeCB = %d, its dims give %lld", who, name, i, w.volumeCB, vol / 2);
    MUGIQ_REQUIRE(w.stride >= w.volumeCB && w.parity_offset >= (int64_t)2 * w.nColor * w.stride && w.stride == f[0].stride && w.parity_offset == f[0].parity_offset,
                  "%s: %s vector %d: stride / parity_offset (one for all %s vectors)", who, name, i, name);
    const MugiqHipCoarseField &g = like ? *like : f[0];
    MUGIQ_REQUIRE(w.nColor == g.nColor && w.X[0] == g.X[0] && w.X[1] == g.X[1] && w.X[2] == g.X[2] && w.X[3] == g.X[3],
                  "%s: %s vector %d differs in nColor or lattice from the first vector of the call", who, name, i);
  }
  return MUGIQ_HIP_SUCCESS;
}

int gram_nchunks(int64_t total) { return (int)((total + kGramChunk - 1) / kGramChunk); }

// G_h[mA][mB] (complex, row-major) = <a_i, b_j>; validated arguments.  One blocking read
int coarse_gram(double *G_h, const MugiqHipCoarseField *a, int mA, const MugiqHipCoarseField *b, int mB, hipStream_t s) {
  std::vector<const void *> host((size_t)mA + mB);
  for (int i = 0; i < mA; i++) host[i] = a[i].data;
  for (int j = 0; j < mB; j++) host[mA + j] = b[j].data;
  void *tab = nullptr;
  if (int st = upload_table(&tab, host.data(), host.size() * sizeof(void *), s)) return st;
  GramArgs A;
  A.tab = static_cast<const void *const *>(tab);
  A.mA = mA, A.mB = mB;
  A.ga = vec_geom(a[0]), A.gb = vec_geom(b[0]);
  const int nChunks = gram_nchunks(A.ga.total), nEntries = mA * mB;
  void *ws = nullptr;
  if (int st = stream_workspace(&ws, sizeof(Z) * (size_t)nEntries * ((size_t)nChunks + 1), s)) return st;
  A.partial = static_cast<Z *>(ws);
  Z *G_d = A.partial + (size_t)nEntries * nChunks;
  hipLaunchKernelGGL(coarse_gram_kernel, dim3((unsigned)nChunks, (unsigned)((mA + 31) / 32), (unsigned)((mB + 31) / 32)), dim3(256), 0, s, A);
  MUGIQ_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(coarse_gram_sum_kernel, dim3((unsigned)((nEntries + 255) / 256)), dim3(256), 0, s, A.partial, nChunks, nEntries, G_d);
  MUGIQ_CHECK_HIP(hipGetLastError());
  MUGIQ_CHECK_HIP(hipMemcpyAsync(G_h, G_d, sizeof(Z) * (size_t)nEntries, hipMemcpyDeviceToHost, s));
  MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
  return MUGIQ_HIP_SUCCESS;
}

// out_j = sum_i in_i Z[i][j]; Z_h[mIn][mOut] complex row-major; validated arguments
int coarse_rotate(const MugiqHipCoarseField *out, int mOut, const MugiqHipCoarseField *in, int mIn, const double *Z_h, hipStream_t s) {
  const int mInPad = (mIn + 3) & ~3, ldz = (mOut + kRotOut - 1) / kRotOut * kRotOut;
  const size_t nPtr = (size_t)mIn + mOut, ptrBytes = align256(nPtr * sizeof(void *)), zDoubles = (size_t)mInPad * ldz;
  std::vector<unsigned char> host(ptrBytes + 2 * zDoubles * sizeof(double), 0);
  const void **hp = reinterpret_cast<const void **>(host.data());
  for (int i = 0; i < mIn; i++) hp[i] = in[i].data;
  for (int j = 0; j < mOut; j++) hp[mIn + j] = out[j].data;
  double *zr = reinterpret_cast<double *>(host.data() + ptrBytes), *zi = zr + zDoubles;
  for (int i = 0; i < mIn; i++)
    for (int j = 0; j < mOut; j++) {
      zr[(size_t)i * ldz + j] = Z_h[2 * ((size_t)i * mOut + j)];
      zi[(size_t)i * ldz + j] = Z_h[2 * ((size_t)i * mOut + j) + 1];
    }
  void *tab = nullptr;
  if (int st = upload_table(&tab, host.data(), host.size(), s)) return st;
  RotArgs A;
  A.tab = static_cast<const void *const *>(tab);
  A.zre = reinterpret_cast<const double *>(static_cast<unsigned char *>(tab) + ptrBytes);
  A.zim = A.zre + zDoubles;
  A.mIn = mIn, A.mOut = mOut, A.mInPad = mInPad, A.ldz = ldz;
  A.gi = vec_geom(in[0]), A.go = vec_geom(out[0]);
  const int64_t perGroup = (int64_t)kRotWaves * kRotElems;
  hipLaunchKernelGGL(coarse_rotate_kernel, dim3((unsigned)((A.gi.total + perGroup - 1) / perGroup), (unsigned)(ldz / kRotOut)), dim3(64 * kRotWaves), 0, s, A);
  MUGIQ_CHECK_HIP(hipGetLastError());
  return MUGIQ_HIP_SUCCESS;
}

int check_eig_param(const MugiqHipCoarseEigParam *p, const char *who) {
  MUGIQ_REQUIRE(p->nKr >= kEigBlock && p->nKr % kEigBlock == 0 && p->nKr <= kEigMaxKr, "%s: nKr = %d must be a multiple of %d in [%d, %d]", who, p->nKr, kEigBlock,
                kEigBlock, kEigMaxKr);
  MUGIQ_REQUIRE(p->nConv >= 1 && p->nConv < p->nKr, "%s: nConv = %d must be in [1, nKr = %d)", who, p->nConv, p->nKr);
  MUGIQ_REQUIRE(p->tol > 0.0 && p->maxIter >= 0, "%s: tol = %g must be positive and maxIter = %d non-negative", who, p->tol, p->maxIter);
  MUGIQ_REQUIRE(p->polyDeg >= 1, "%s: polyDeg = %d must be >= 1", who, p->polyDeg);
  MUGIQ_REQUIRE(p->nOrtho >= 1 && p->nOrtho <= 3, "%s: nOrtho = %d must be in [1, 3]", who, p->nOrtho);
  MUGIQ_REQUIRE(p->rankTol >= 0.0 && p->rankTol <= 1.0, "%s: rankTol = %g must be in [0, 1]", who, p->rankTol);
  MUGIQ_REQUIRE(!(p->aMin > 0.0 && p->aMax > 0.0) || p->aMin < p->aMax, "%s: aMin = %g must be below aMax = %g", who, p->aMin, p->aMax);
  MUGIQ_REQUIRE(std::isfinite(p->aMin) && std::isfinite(p->aMax), "%s: aMin / aMax not finite", who);
  return MUGIQ_HIP_SUCCESS;
}

// MUGIQ_HIP_EIG_PACK_IN_STEP (read once per call of the grid solver): 1 the recurrence kernel writes the send faces of the next
// application (chebyshev_step_pack_kernel), 0 the plain step kernel and a separate face_pack_kernel per face.  The same bits either way
bool eig_pack_in_step() {
  const char *e = getenv("MUGIQ_HIP_EIG_PACK_IN_STEP");
  return e ? atoi(e) != 0 : kEigPackInStepDefault;
}

struct DeviceSlab {
  void *p = nullptr;
  ~DeviceSlab() {
    if (p) (void)hipFree(p);
  }
};


// the state of one call of mugiq_hip_coarse_eigensolve
struct EigRun {
  const MugiqHipCoarseOperator *op = nullptr;
  int opType = 0;
  const MugiqHipCoarseEigParam *prm = nullptr;
  MugiqHipCoarseEigInfo *info = nullptr;
  hipStream_t s = nullptr;
  const char *who = "";
  int nKr = 0;
  int64_t pitch = 0, total = 0;                    // complex elements between the vectors of a basis; in a vector
  std::vector<MugiqHipCoarseField> base[3], ring;  // three bases of nKr packed vectors, 24 more
  double *scal_d = nullptr;                        // [theta nKr | r^2 nKr | partial nKr chunks]
  int nChunks = 0;
  double aMax = 0.0, aMinLast = 0.0, dense = 0.0;
  std::vector<double> G, R, Rinv, Zrot, theta, r;
  std::vector<char> conv;
  int nLocked = 0;
  int q = 0, w = 1, sp = 2;  // which base holds Q, W = A Q and the spare
  const MugiqHipCoarseField *start = nullptr;  // the caller's start vectors
  bool estimated = false;                      // the power estimate of aMax has run

  // a rank of a process grid (mugiq_hip_coarse_eigensolve_grid; all unset: one domain).  The lattice is touched in three places: apply
  // exchanges faces, gram and the residual norms are added over the ranks; the rest is local or repeated on identical input
  const MugiqHipComm *comm = nullptr;
  bool multi = false;  // more than one rank: sums go through sum_over_ranks
  const MugiqHipCoarseHalo *halo = nullptr;
  int part[4] = {0, 0, 0, 0};
  bool partitioned = false;
  bool packInStep = false;  // the recurrence kernel writes the send faces of the next application
  bool facesPacked = false;  // ... and has done so for the vectors the next apply takes
  CoarseGridLayout layout{};
  unsigned char *wsBase = nullptr;  // the per-stream workspace, reserved once for the largest request of the call
  MugiqHipCoarseEigGridInfo ginfo{};

  static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
  Z *body(const MugiqHipCoarseField &f) const { return static_cast<Z *>(f.data); }

  int rank_sum(double *v, size_t n) {
    if (!multi) return MUGIQ_HIP_SUCCESS;
    std::vector<double> c(v, v + n);
    ginfo.rankSums++;
    if (int st = sum_over_ranks(comm, c)) return st;
    std::copy(c.begin(), c.end(), v);
    return MUGIQ_HIP_SUCCESS;
  }
  int apply(const MugiqHipCoarseField *dst, const MugiqHipCoarseField *src, int n) {
    info->opBlocks += (n + kEigBlock - 1) / kEigBlock;
    if (!partitioned) return coarse_apply(dst, src, n, op, opType, 1.0, s);
    const bool packed = facesPacked;
    facesPacked = false;
    CoarseGridCounts counts;
    const int st = coarse_apply_grid(dst, src, n, op, halo, part, opType, 1.0, comm, s, packed, &counts);
    ginfo.exchanges += counts.exchanges, ginfo.packLaunches += counts.packLaunches;
    if (packed) ginfo.stepPacked++;
    return st;
  }
  int gram(const MugiqHipCoarseField *a, int mA, const MugiqHipCoarseField *b, int mB) {
    info->hostReads++;
    if (int st = coarse_gram(G.data(), a, mA, b, mB, s)) return st;
    return rank_sum(G.data(), (size_t)2 * mA * mB);
  }

  // nOrtho rounds of Cholesky QR of the nKr vectors Y (a base, or the caller's start vectors), written to the bases f0 and f1 in turn,
  // neither of which holds Y.  *res: the base the result is in, -1 if no round was made; *rank: a pivot failed and ended the call
  int orth(const MugiqHipCoarseField *Y, int f0, int f1, int *res, bool *rank) {
    *rank = false;
    *res = -1;
    for (int round = 0; round < prm->nOrtho; round++) {
      if (int st = gram(Y, nKr, Y, nKr)) return st;
      for (int j = 0; j < nKr; j++)
        if (!std::isfinite(G[2 * ((size_t)j * nKr + j)]))
          return set_error(MUGIQ_HIP_ERROR_HIP, "%s: the Gram matrix of the basis has a non-finite diagonal entry (column %d): the filter overflowed or an input is not finite",
                           who, j);
      const auto t0 = std::chrono::steady_clock::now();
      int st = cholesky_upper(nKr, G.data(), R.data(), prm->rankTol, nullptr, nullptr, who);
      if (st == MUGIQ_HIP_SUCCESS) st = upper_inverse(nKr, R.data(), Rinv.data(), who);
      dense += since(t0);
      if (st == MUGIQ_HIP_ERROR_INVALID_ARGUMENT) {
        *rank = true;
        return MUGIQ_HIP_SUCCESS;
      }
      if (st) return st;
      const int dst = (round & 1) ? f1 : f0;
      if ((st = coarse_rotate(base[dst].data(), nKr, Y, nKr, Rinv.data(), s))) return st;
      *res = dst;
      Y = base[dst].data();
    }
    return MUGIQ_HIP_SUCCESS;
  }

  // W = A Q, H = Q^dag W, H = Z Theta Z^dag, Q <- Q Z, W <- W Z, r_i = ||W_i - theta_i Q_i||; aMax repaired, conv and nLocked set
  int rayleigh_ritz() {
    int st;
    if ((st = apply(base[w].data(), base[q].data(), nKr))) return st;
    if ((st = gram(base[q].data(), nKr, base[w].data(), nKr))) return st;
    const auto t0 = std::chrono::steady_clock::now();
    st = hermitian_eigh(nKr, G.data(), theta.data(), Zrot.data(), who);  // Hermitises: (H + H^dag) / 2
    dense += since(t0);
    if (st == MUGIQ_HIP_ERROR_INVALID_ARGUMENT) return set_error(MUGIQ_HIP_ERROR_HIP, "%s: the Rayleigh-Ritz matrix is not finite", who);
    // (status 5 of this call means "maxIter exhausted, outputs filled"; a QL iteration that gives up is neither)
    if (st == MUGIQ_HIP_ERROR_NOT_CONVERGED)
      return set_error(MUGIQ_HIP_ERROR_HIP, "%s: the host's QL iteration on the Rayleigh-Ritz matrix did not converge; the outputs are not filled", who);
    if (st) return st;
    if ((st = coarse_rotate(base[sp].data(), nKr, base[q].data(), nKr, Zrot.data(), s))) return st;
    if ((st = coarse_rotate(base[q].data(), nKr, base[w].data(), nKr, Zrot.data(), s))) return st;
    const int oldq = q;
    q = sp, sp = w, w = oldq;
    // residuals
    double *theta_d = scal_d, *r2_d = scal_d + nKr, *partial_d = scal_d + 2 * nKr;
    MUGIQ_CHECK_HIP(hipMemcpyAsync(theta_d, theta.data(), sizeof(double) * nKr, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(residual_partial_kernel, dim3((unsigned)nChunks, (unsigned)nKr), dim3(kEwThreads), 0, s, body(base[w][0]), body(base[q][0]), theta_d, pitch, total,
                       partial_d);
    MUGIQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(residual_sum_kernel, dim3((unsigned)((nKr + kEwThreads - 1) / kEwThreads)), dim3(kEwThreads), 0, s, partial_d, nChunks, nKr, r2_d);
    MUGIQ_CHECK_HIP(hipGetLastError());
    MUGIQ_CHECK_HIP(hipMemcpyAsync(r.data(), r2_d, sizeof(double) * nKr, hipMemcpyDeviceToHost, s));
    MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
    info->hostReads++;
    if ((st = rank_sum(r.data(), (size_t)nKr))) return st;
    for (int i = 0; i < nKr; i++) r[i] = std::sqrt(r[i]);
    if (theta[nKr - 1] > aMax) {
      aMax = kAmaxMargin * theta[nKr - 1];
      // a GIVEN aMax that a Ritz value exceeds is shown to be wrong.  The Ritz value repairs it only as far as the basis reaches, and a
      // filter whose aMax is still below lambda_max amplifies the top of the spectrum; so the power estimate runs after all, once
      if (!estimated) {
        double est = 0.0;
        if ((st = estimate_amax(&est))) return st;
        aMax = std::max(aMax, est);
      }
    }
    for (int i = 0; i < nKr; i++) conv[i] = r[i] <= prm->tol * aMax;
    nLocked = 0;
    while (nLocked + kEigBlock <= nKr && std::all_of(conv.begin() + nLocked, conv.begin() + nLocked + kEigBlock, [](char c) { return c != 0; })) nLocked += kEigBlock;
    return MUGIQ_HIP_SUCCESS;
  }

  // pack: `out` is the input of another application of this block, whose send faces the step writes (a grid with packInStep)
  int cheb_step(const MugiqHipCoarseField *out, const MugiqHipCoarseField *y, const MugiqHipCoarseField *t, const MugiqHipCoarseField *prev, double alpha, double beta,
                bool pack) {
    ChebArgs A;
    A.out = body(out[0]), A.y = body(y[0]), A.t = body(t[0]), A.prev = prev ? body(prev[0]) : nullptr;
    A.pitch = pitch, A.total = total, A.alpha = alpha, A.beta = beta;
    if (pack) {
      ChebPackArgs P;
      P.c = A;
      P.volumeCB = op->volumeCB, P.rows = 2 * op->nVec;
      for (int d = 0; d < 4; d++) {
        P.X[d] = op->X[d], P.part[d] = part[d], P.faceCB[d] = layout.faceCB[d];
        for (int h = 0; h < 2; h++) P.send[d][h] = part[d] ? reinterpret_cast<Z *>(wsBase + layout.send[d][h]) : nullptr;
      }
      const int waves = kEwThreads / 64, chunks = (P.rows + waves * kStepRows - 1) / (waves * kStepRows);
      hipLaunchKernelGGL(chebyshev_step_pack_kernel, dim3((unsigned)((P.volumeCB + 63) / 64), 2 * kEigBlock, (unsigned)chunks), dim3(kEwThreads), 0, s, P);
      MUGIQ_CHECK_HIP(hipGetLastError());
      facesPacked = true;
      return MUGIQ_HIP_SUCCESS;
    }
    hipLaunchKernelGGL(chebyshev_step_kernel, dim3((unsigned)std::min<int64_t>(1024, (total + kEwThreads - 1) / kEwThreads), kEigBlock), dim3(kEwThreads), 0, s, A);
    MUGIQ_CHECK_HIP(hipGetLastError());
    return MUGIQ_HIP_SUCCESS;
  }

  // Q_j <- T_deg(A) Q_j for the block of 8 columns from j0, in place; the product A t goes through the first 8 vectors of the spare base
  int filter_block(int j0, double aMin) {
    const double d1 = 2.0 / (aMax - aMin), d2 = -(aMax + aMin) / (aMax - aMin);
    const MugiqHipCoarseField *Qb = base[q].data() + j0, *Y = base[sp].data();
    const int deg = prm->polyDeg;
    const MugiqHipCoarseField *prev = Qb, *cur = Qb;
    for (int k = 1; k <= deg; k++) {
      int st;
      if ((st = apply(Y, cur, kEigBlock))) return st;
      const MugiqHipCoarseField *out = k == deg ? Qb : ring.data() + kEigBlock * ((k - 1) % 3);
      const bool pack = partitioned && packInStep && k < deg;  // only a step that feeds another application of the block
      if (k == 1) st = cheb_step(out, Y, cur, nullptr, d1, d2, pack);
      else st = cheb_step(out, Y, cur, prev, 2.0 * d1, 2.0 * d2, pack);
      if (st) return st;
      prev = cur, cur = out;
    }
    return MUGIQ_HIP_SUCCESS;
  }

  // *out = 1.1 max_j <x_j, A x_j> after kPowerSteps power steps on the first 8 start vectors, each normalised after each step.  Works in
  // the 24 vectors of the recurrence, which are free outside a filter, so that it can run beside a basis
  int estimate_amax(double *out) {
    estimated = true;
    const MugiqHipCoarseField *x = start, *y = ring.data();
    std::vector<double> D(2 * kEigBlock * kEigBlock);
    for (int step = 0; step <= kPowerSteps; step++) {
      int st;
      if ((st = apply(y, x, kEigBlock))) return st;
      if (step == kPowerSteps) {
        if ((st = gram(x, kEigBlock, y, kEigBlock))) return st;
        double best = 0.0;
        for (int j = 0; j < kEigBlock; j++) best = std::max(best, G[2 * (j * kEigBlock + j)]);
        if (!(best > 0.0) || !std::isfinite(best))
          return set_error(MUGIQ_HIP_ERROR_HIP, "%s: the power iteration gave max <x, A x> = %g: the operator or the start vectors are zero or not finite", who, best);
        *out = kAmaxMargin * best;
        return MUGIQ_HIP_SUCCESS;
      }
      if ((st = gram(y, kEigBlock, y, kEigBlock))) return st;
      std::fill(D.begin(), D.end(), 0.0);
      for (int j = 0; j < kEigBlock; j++) {
        const double n2 = G[2 * (j * kEigBlock + j)];
        if (!(n2 > 0.0) || !std::isfinite(n2))
          return set_error(MUGIQ_HIP_ERROR_HIP, "%s: power step %d left ||A x_%d||^2 = %g", who, step, j, n2);
        D[2 * (j * kEigBlock + j)] = 1.0 / std::sqrt(n2);
      }
      const MugiqHipCoarseField *xn = ring.data() + kEigBlock * (1 + (step & 1));
      if ((st = coarse_rotate(xn, kEigBlock, y, kEigBlock, D.data(), s))) return st;
      x = xn;
    }
    return MUGIQ_HIP_SUCCESS;
  }
};

}  // namespace
}  // namespace mugiq

using namespace mugiq;

extern "C" {

int mugiq_hip_coarse_gram(double *G_h, const MugiqHipCoarseField *a_h, int mA, const MugiqHipCoarseField *b_h, int mB, const MugiqHipComm *comm, void *stream) {
  const char *who = "coarseGram";
  MUGIQ_REQUIRE(G_h != nullptr && a_h != nullptr && b_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(mA >= 1 && mB >= 1 && mA <= 4096 && mB <= 4096, "%s: mA = %d and mB = %d must be in [1, 4096]", who, mA, mB);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = check_fields(a_h, mA, nullptr, who, "a"))) return st;
  if ((st = check_fields(b_h, mB, a_h, who, "b"))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  return coarse_gram(G_h, a_h, mA, b_h, mB, s);
}

int mugiq_hip_coarse_rotate(const MugiqHipCoarseField *out_h, int mOut, const MugiqHipCoarseField *in_h, int mIn, const double *Z_h, const MugiqHipComm *comm,
                            void *stream) {
  const char *who = "coarseRotate";
  MUGIQ_REQUIRE(out_h != nullptr && in_h != nullptr && Z_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(mIn >= 1 && mOut >= 1 && mIn <= 4096 && mOut <= 4096, "%s: mIn = %d and mOut = %d must be in [1, 4096]", who, mIn, mOut);
  int st;
  if ((st = check_single_domain(comm, who))) return st;
  if ((st = check_fields(in_h, mIn, nullptr, who, "in"))) return st;
  if ((st = check_fields(out_h, mOut, in_h, who, "out"))) return st;
  for (int j = 0; j < mOut; j++) {
    uintptr_t a0, a1;
    coarse_span(out_h[j], &a0, &a1);
    for (int i = 0; i < mIn; i++) {
      uintptr_t b0, b1;
      coarse_span(in_h[i], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: out vector %d overlaps in vector %d (the rotation is out of place)", who, j, i);
    }
    for (int i = 0; i < j; i++) {
      uintptr_t b0, b1;
      coarse_span(out_h[i], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: out vector %d overlaps out vector %d", who, j, i);
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  return coarse_rotate(out_h, mOut, in_h, mIn, Z_h, s);
}

int mugiq_hip_coarse_eig_param_default(MugiqHipCoarseEigParam *p) {
  MUGIQ_REQUIRE(p != nullptr, "coarseEigParamDefault: param is NULL");
  // the members the reference's tests/eigensolve.cpp:251-289 fills from QUDA's flags (eig_nConv, eig_nKr, eig_tol, eig_max_restarts,
  // eig_poly_deg, eig_amin, eig_amax); it fixes no values, so every number below is this project's
  p->nConv = 200;     // the N_ev of the flagship workload
  p->nKr = 256;       // the next multiple of 8 with a quarter to spare: first guess, NOT tuned
  p->tol = 1e-10;     // first guess, NOT tuned: the criterion here is r_i <= tol aMax, not QUDA's
  p->maxIter = 100;   // first guess, NOT tuned
  p->polyDeg = 20;    // first guess, NOT tuned
  p->aMin = 0.0;      // <= 0: adaptive (the largest Ritz value of the previous Rayleigh-Ritz step)
  p->aMax = 0.0;      // <= 0: estimated by 20 power steps (QUDA: 100), margin 1.1 (QUDA's)
  p->nOrtho = 2;      // "twice is enough"
  p->rankTol = 1e-14; // first guess, NOT tuned: filtered columns differ in norm by many orders, and the pivots are measured against the largest
  return MUGIQ_HIP_SUCCESS;
}

// mugiq_hip_coarse_eigensolve (gridInfo NULL: one domain, halo not looked at) and mugiq_hip_coarse_eigensolve_grid
static int coarse_eigensolve(const MugiqHipCoarseField *evecs_h, const MugiqHipCoarseField *start_h, const MugiqHipCoarseOperator *op,
                             const MugiqHipCoarseHalo *halo, int opType, const MugiqHipCoarseEigParam *param, double *theta_h, double *residual_h,
                             double *sigma_h, MugiqHipCoarseEigInfo *info, MugiqHipCoarseEigGridInfo *gridInfo, const MugiqHipComm *comm, void *stream) {
  const bool grid = gridInfo != nullptr;
  const char *who = grid ? "coarseEigensolveGrid" : "coarseEigensolve";
  MUGIQ_REQUIRE(evecs_h != nullptr && start_h != nullptr && param != nullptr && theta_h != nullptr && residual_h != nullptr && sigma_h != nullptr && info != nullptr,
                "%s: NULL argument", who);
  int st, part[4] = {0, 0, 0, 0};
  if ((st = check_eig_param(param, who))) return st;
  if (grid) {
    MUGIQ_REQUIRE(comm != nullptr, "%s: comm is NULL (the single-domain call is mugiq_hip_coarse_eigensolve)", who);
    if ((st = check_coarse_grid(comm, op, halo, part, true, who))) return st;
  } else {
    if ((st = check_single_domain(comm, who))) return st;
    if ((st = validate_coarse_operator(op, who))) return st;
  }
  const int nRanks = grid ? comm->size : 1;
  MUGIQ_REQUIRE(valid_op(opType), "%s: opType %d is none of M, Mdag, MdagM, MMdag, H", who, opType);
  if (!normal_op(opType))
    return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: opType %d: the solver needs a Hermitian positive operator, MdagM or MMdag", who, opType);
  if (op->precision != 8) return set_error(MUGIQ_HIP_ERROR_UNSUPPORTED, "%s: the coarse operator has precision %d: the eigensolver is fp64 only", who, op->precision);
  const int nKr = param->nKr, nConv = param->nConv;
  if ((st = check_fields(start_h, nKr, nullptr, who, "start"))) return st;
  if ((st = check_fields(evecs_h, nConv, nullptr, who, "evecs"))) return st;
  if ((st = validate_coarse_vectors(start_h, nKr, op, who, "start"))) return st;
  if ((st = validate_coarse_vectors(evecs_h, nConv, op, who, "evecs"))) return st;
  const int64_t total = (int64_t)2 * 2 * op->nVec * op->volumeCB;
  MUGIQ_REQUIRE(nKr <= total * nRanks, "%s: nKr = %d exceeds the dimension %lld of the coarse space", who, nKr, (long long)(total * nRanks));
  for (int j = 0; j < nConv; j++) {
    uintptr_t a0, a1;
    coarse_span(evecs_h[j], &a0, &a1);
    for (int i = 0; i < nKr; i++) {
      uintptr_t b0, b1;
      coarse_span(start_h[i], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: eigenvector %d overlaps start vector %d", who, j, i);
    }
    for (int i = 0; i < j; i++) {
      uintptr_t b0, b1;
      coarse_span(evecs_h[i], &b0, &b1);
      MUGIQ_REQUIRE(!(a0 < b1 && b0 < a1), "%s: eigenvector %d overlaps eigenvector %d", who, j, i);
    }
  }

  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  *info = MugiqHipCoarseEigInfo{};
  if (gridInfo) *gridInfo = MugiqHipCoarseEigGridInfo{};
  EigRun run;
  run.op = op, run.opType = opType, run.prm = param, run.info = info, run.s = s, run.who = who, run.nKr = nKr, run.total = total;
  run.nChunks = gram_nchunks(total);
  if (grid) {
    run.comm = comm, run.halo = halo, run.multi = comm->size > 1;
    for (int d = 0; d < 4; d++) run.part[d] = part[d], run.partitioned |= part[d] != 0;
  }
  if (run.partitioned) {
    // the per-stream workspace, once, for the largest request of the call (the Gram matrix of a basis; the faces and the intermediate of
    // an application of 8 vectors): it stays where it is, so the recurrence kernel knows the send buffers of the next application
    run.packInStep = eig_pack_in_step();
    coarse_grid_layout(&run.layout, op, part, opType, kEigBlock);
    void *ws = nullptr;
    if ((st = stream_workspace(&ws, std::max(run.layout.bytes, sizeof(Z) * (size_t)nKr * nKr * ((size_t)run.nChunks + 1)), s))) return st;
    run.wsBase = static_cast<unsigned char *>(ws);
  }
  // work memory: three bases of nKr packed vectors, 24 vectors for the Chebyshev recurrence, and the scalars of the residual kernels
  const size_t vecBytes = align256((size_t)total * sizeof(Z)), nWork = (size_t)3 * nKr + 3 * kEigBlock;
  const size_t scalBytes = align256(sizeof(double) * (size_t)nKr * (2 + run.nChunks));
  run.pitch = (int64_t)(vecBytes / sizeof(Z));
  DeviceSlab slab;
  if (hipMalloc(&slab.p, vecBytes * nWork + scalBytes) != hipSuccess) {
    slab.p = nullptr;
    (void)hipGetLastError();
    return set_error(MUGIQ_HIP_ERROR_HIP, "%s: no device memory for %zu work vectors of %zu bytes", who, nWork, vecBytes);
  }
  auto carve = [&](size_t k) {
    MugiqHipCoarseField f = start_h[0];
    f.data = static_cast<unsigned char *>(slab.p) + vecBytes * k;
    f.stride = op->volumeCB;
    f.parity_offset = (int64_t)2 * op->nVec * op->volumeCB;
    return f;
  };
  for (int b = 0; b < 3; b++) {
    run.base[b].resize(nKr);
    for (int i = 0; i < nKr; i++) run.base[b][i] = carve((size_t)b * nKr + i);
  }
  run.ring.resize(3 * kEigBlock);
  for (int i = 0; i < 3 * kEigBlock; i++) run.ring[i] = carve((size_t)3 * nKr + i);
  run.scal_d = reinterpret_cast<double *>(static_cast<unsigned char *>(slab.p) + vecBytes * nWork);
  run.G.assign((size_t)2 * nKr * nKr, 0.0), run.R = run.G, run.Rinv = run.G, run.Zrot = run.G;
  run.theta.assign(nKr, 0.0), run.r.assign(nKr, 0.0), run.conv.assign(nKr, 0);

  // the outputs from the first nConv columns of `Q` (a base, or the start vectors if nothing was orthonormalised), and the info
  auto finish = [&](const MugiqHipCoarseField *Q, int status, const char *what) -> int {
    std::vector<double> I((size_t)2 * nConv * nConv, 0.0);
    for (int j = 0; j < nConv; j++) I[2 * ((size_t)j * nConv + j)] = 1.0;
    int e;
    if ((e = coarse_rotate(evecs_h, nConv, Q, nConv, I.data(), s))) return e;
    if ((e = run.gram(evecs_h, nConv, evecs_h, nConv))) return e;
    double dev = 0.0;
    for (int i = 0; i < nConv; i++)
      for (int j = 0; j < nConv; j++) {
        const double re = run.G[2 * ((size_t)i * nConv + j)] - (i == j ? 1.0 : 0.0), im = run.G[2 * ((size_t)i * nConv + j) + 1];
        const double d = std::sqrt(re * re + im * im);
        if (d > dev || d != d) dev = d;
      }
    int nc = 0;
    for (int i = 0; i < nConv; i++) {
      theta_h[i] = run.theta[i], residual_h[i] = run.r[i], sigma_h[i] = std::sqrt(std::max(run.theta[i], 0.0));
      nc += run.conv[i] ? 1 : 0;
    }
    info->nConverged = nc;
    info->aMaxUsed = run.aMax, info->aMinLast = run.aMinLast;
    info->orthonormality = dev;
    info->hostDenseSeconds = run.dense;
    if (gridInfo) *gridInfo = run.ginfo;
    MUGIQ_CHECK_HIP(hipStreamSynchronize(s));
    if (status == MUGIQ_HIP_ERROR_INVALID_ARGUMENT)
      return set_error(status, "%s: %s: a pivot of the Cholesky QR fell to rankTol = %.3e x the largest squared norm: the basis is dependent (outputs and info are filled)", who,
                       what, param->rankTol);
    if (status == MUGIQ_HIP_ERROR_NOT_CONVERGED)
      return set_error(status, "%s: %d of %d pairs converged to tol = %.3e x aMax = %.3e within maxIter = %d (outputs and info are filled)", who, nc, nConv, param->tol,
                       run.aMax, param->maxIter);
    return status;
  };

  run.aMax = param->aMax;
  run.aMinLast = param->aMin;
  run.start = start_h;
  if (!(run.aMax > 0.0) && (st = run.estimate_amax(&run.aMax))) return st;
  bool rank = false;
  int res = -1;
  if ((st = run.orth(start_h, 0, 1, &res, &rank))) return st;
  if (rank) return finish(res < 0 ? start_h : run.base[res].data(), MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "the start vectors");
  run.q = res, run.w = (res + 1) % 3, run.sp = (res + 2) % 3;
  if ((st = run.rayleigh_ritz())) return st;
  auto done = [&]() { return std::all_of(run.conv.begin(), run.conv.begin() + nConv, [](char c) { return c != 0; }); };
  while (!done() && info->iters < param->maxIter) {
    run.aMinLast = param->aMin > 0.0 ? param->aMin : run.theta[nKr - 1];
    if (!(run.aMinLast < run.aMax))
      return set_error(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "%s: aMin = %g is not below aMax = %g", who, run.aMinLast, run.aMax);
    for (int j0 = run.nLocked; j0 < nKr; j0 += kEigBlock)
      if ((st = run.filter_block(j0, run.aMinLast))) return st;
    if ((st = run.orth(run.base[run.q].data(), run.w, run.sp, &res, &rank))) return st;
    if (rank) return finish(run.base[res < 0 ? run.q : res].data(), MUGIQ_HIP_ERROR_INVALID_ARGUMENT, "the filtered basis");
    run.q = res, run.w = (res + 1) % 3, run.sp = (res + 2) % 3;
    if ((st = run.rayleigh_ritz())) return st;
    info->iters++;
  }
  return finish(run.base[run.q].data(), done() ? MUGIQ_HIP_SUCCESS : MUGIQ_HIP_ERROR_NOT_CONVERGED, "");
}

int mugiq_hip_coarse_eigensolve(const MugiqHipCoarseField *evecs_h, const MugiqHipCoarseField *start_h, const MugiqHipCoarseOperator *op, int opType,
                                const MugiqHipCoarseEigParam *param, double *theta_h, double *residual_h, double *sigma_h, MugiqHipCoarseEigInfo *info,
                                const MugiqHipComm *comm, void *stream) {
  return coarse_eigensolve(evecs_h, start_h, op, nullptr, opType, param, theta_h, residual_h, sigma_h, info, nullptr, comm, stream);
}

int mugiq_hip_coarse_eigensolve_grid(const MugiqHipCoarseField *evecs_h, const MugiqHipCoarseField *start_h, const MugiqHipCoarseOperator *op,
                                     const MugiqHipCoarseHalo *halo, int opType, const MugiqHipCoarseEigParam *param, double *theta_h,
                                     double *residual_h, double *sigma_h, MugiqHipCoarseEigInfo *info, MugiqHipCoarseEigGridInfo *gridInfo,
                                     const MugiqHipComm *comm, void *stream) {
  MUGIQ_REQUIRE(gridInfo != nullptr, "coarseEigensolveGrid: NULL argument");
  return coarse_eigensolve(evecs_h, start_h, op, halo, opType, param, theta_h, residual_h, sigma_h, info, gridInfo, comm, stream);
}

int mugiq_hip_coarse_gram_grid(double *G_h, const MugiqHipCoarseField *a_h, int mA, const MugiqHipCoarseField *b_h, int mB, const MugiqHipComm *comm,
                               void *stream) {
  const char *who = "coarseGramGrid";
  MUGIQ_REQUIRE(G_h != nullptr && a_h != nullptr && b_h != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(comm != nullptr, "%s: comm is NULL (the single-domain call is mugiq_hip_coarse_gram)", who);
  MUGIQ_REQUIRE(mA >= 1 && mB >= 1 && mA <= 4096 && mB <= 4096, "%s: mA = %d and mB = %d must be in [1, 4096]", who, mA, mB);
  int st, part[4];
  if ((st = check_comm(comm, part, true, who))) return st;
  if ((st = check_fields(a_h, mA, nullptr, who, "a"))) return st;
  if ((st = check_fields(b_h, mB, a_h, who, "b"))) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((st = debug_poison_lds_if_asked(s))) return st;
  if ((st = coarse_gram(G_h, a_h, mA, b_h, mB, s))) return st;
  if (comm->size > 1) {
    std::vector<double> c(G_h, G_h + (size_t)2 * mA * mB);
    if ((st = sum_over_ranks(comm, c))) return st;
    std::copy(c.begin(), c.end(), G_h);
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // extern "C"
