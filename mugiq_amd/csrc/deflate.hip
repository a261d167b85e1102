// Low-mode deflation of solutions: dst_r <- dst_r - sum_n v_n sigma_n^-1 c_nr,  c_nr = sum_x v_n(x)^dag G src_r(x), G = g5 | 1.
// The deflated stochastic part of a disconnected loop: phi_r = x_r - (low-mode part of M^-1) xi_r.
//
// Both passes walk the fields in SEGMENTS: 64 consecutive complex elements of one plane of one parity (FLOAT2: 64 sites of one
// component; FLOAT4: 32 sites of one component pair).  Every field of a call has the same order, stride and parity offset, so a
// segment sits at the same element offset in all of them, pads are never part of one, and gamma5 is one sign per segment
// (components 0-5 are spins 0-1: +1; 6-11: -1).
//
//   pass 1  deflate_overlap_kernel: a workgroup owns a chunk of segments and 64 eigenvectors (one per lane); each segment of those
//           eigenvectors is staged through LDS (coalesced, transposed) and each wave contracts it with a quarter of the block of
//           right-hand sides, loaded once per segment (lane = element) and broadcast element by element with v_readlane.  Per-chunk partial sums (fp64) go to
//           the stream workspace; deflate_reduce_kernel adds them in chunk order (no atomics: bitwise reproducible) into C and
//           D = diag(1/sigma) C.
//   pass 2  deflate_update_kernel: one element per lane, all eigenvectors streamed (coalesced), D read through scalar loads, each
//           dst element read and written once, fp32 rounded once.
// Right-hand sides are handled in blocks of up to 16 (RB = 4, 8, 12, 16 instances); every eigenvector is read once per pass and block.
#include "internal.h"

#include <algorithm>
#include <vector>

namespace mugiq {
namespace {

constexpr int kSeg = 64;    // complex elements per segment
constexpr int kNB = 64;     // eigenvectors per pass-1 workgroup (one per lane)
constexpr int kRBMax = 16;  // right-hand sides per block

struct DeflateGeom {
  int64_t parity_offset;  // complex elements
  int stride, volumeCB;
  int cpp;                // complex elements per site and plane: 1 (FLOAT2) | 2 (FLOAT4)
  int planes;             // 12 | 6
  int segsPerPlane, nSeg;
};

// element i of a complex array, loaded or stored through the global / constant address space (vector types: Cplx<F> has no
// copy operations across address spaces)
template <typename F> __device__ inline Cplx<F> ld_global(const void *base, int64_t i) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  const vec2 t = *as_global(reinterpret_cast<const vec2 *>(base) + i);
  return Cplx<F>{t.x, t.y};
}
template <typename F> __device__ inline Cplx<F> ld_constant(const void *base, int64_t i) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  const vec2 t = *as_constant(reinterpret_cast<const vec2 *>(base) + i);
  return Cplx<F>{t.x, t.y};
}
template <typename F> __device__ inline void st_global(void *base, int64_t i, F re, F im) {
  typedef F vec2 __attribute__((ext_vector_type(2)));
  vec2 t;
  t.x = re;
  t.y = im;
  *as_global(reinterpret_cast<vec2 *>(base) + i) = t;
}

// the value lane l of the wave holds (l wave-uniform)
__device__ inline double readlane(double x, int l) {
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ inline void seg_place(const DeflateGeom &g, int s, int64_t *off, int *valid, int *plane) {
  const int q = s / g.segsPerPlane;
  const int o = (s - q * g.segsPerPlane) * kSeg;
  const int parity = q / g.planes, j = q - parity * g.planes;
  *off = parity * g.parity_offset + (int64_t)j * g.stride * g.cpp + o;
  *valid = min(kSeg, g.cpp * g.volumeCB - o);
  *plane = j;
}

// partial[chunk][n][RB] = sum over the chunk's segments of conj(v_n) * (G src_r),  r = r0 + w*RB/4 + j  (S = the table from r0)
template <typename FV, typename FS, int RB>
__global__ __launch_bounds__(256) void deflate_overlap_kernel(const void *const *V, const void *const *S, int nEv, int nR, DeflateGeom g,
                                                              int nNB, int segsPerChunk, int gamma5, Cplx<double> *partial) {
  __shared__ Cplx<FV> tile[kNB][kSeg + 1];  // [eigenvector][element], padded against bank conflicts of the column reads
  constexpr int RW = RB / 4;
  const int nb = blockIdx.x % nNB, chunk = blockIdx.x / nNB;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n0 = nb * kNB;
  const auto *Vc = as_constant(V);
  const auto *Sc = as_constant(S);
  Cplx<double> acc[RW];
#pragma unroll
  for (int j = 0; j < RW; j++) acc[j] = Cplx<double>{0.0, 0.0};
  const int s0 = chunk * segsPerChunk, s1 = min(g.nSeg, s0 + segsPerChunk);
  for (int s = s0; s < s1; s++) {
    int64_t off;
    int valid, plane;
    seg_place(g, s, &off, &valid, &plane);
    __syncthreads();  // the previous segment has been consumed
#pragma unroll
    for (int i = 0; i < kNB / 4; i++) {
      const int nl = w + 4 * i, n = n0 + nl;
      Cplx<FV> v{FV(0), FV(0)};
      if (n < nEv && lane < valid) v = ld_global<FV>(Vc[n], off + lane);
      tile[nl][lane] = v;
    }
    // this wave's right-hand sides at element `lane` of the segment, G applied; broadcast below with readlane
    const double sg = (gamma5 && plane >= g.planes / 2) ? -1.0 : 1.0;
    Cplx<double> sl[RW];
#pragma unroll
    for (int j = 0; j < RW; j++) {
      const int r = w * RW + j;
      Cplx<FS> sv{FS(0), FS(0)};
      if (r < nR && lane < valid) sv = ld_global<FS>(Sc[r], off + lane);
      sl[j] = Cplx<double>{sg * (double)sv.re, sg * (double)sv.im};
    }
    __syncthreads();
    for (int e = 0; e < valid; e++) {
      const Cplx<FV> vv = tile[lane][e];
      const double vr = vv.re, vi = vv.im;
#pragma unroll
      for (int j = 0; j < RW; j++) {
        const int r = w * RW + j;
        if (r < nR) {
          const double sr = readlane(sl[j].re, e), si = readlane(sl[j].im, e);
          acc[j].re = fma(vr, sr, acc[j].re);
          acc[j].re = fma(vi, si, acc[j].re);
          acc[j].im = fma(vr, si, acc[j].im);
          acc[j].im = fma(-vi, sr, acc[j].im);
        }
      }
    }
  }
  const int n = n0 + lane;
  if (n < nEv) {
#pragma unroll
    for (int j = 0; j < RW; j++) partial[((int64_t)chunk * nEv + n) * RB + w * RW + j] = acc[j];
  }
}

// C[n][r0 + r] = sum_chunk partial[chunk][n][r] in chunk order;  D[n][r] = C * invSigma[n] (0 for r >= nR)
__global__ __launch_bounds__(256) void deflate_reduce_kernel(const Cplx<double> *partial, int nChunks, int nEv, int RB, int nR, int r0,
                                                             int nVec, const double *invSigma, Cplx<double> *C, Cplx<double> *D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nEv * RB) return;
  const int n = i / RB, r = i - n * RB;
  Cplx<double> c{0.0, 0.0};
  if (r < nR) {
#pragma unroll 8
    for (int k = 0; k < nChunks; k++) {
      const Cplx<double> p = partial[(int64_t)k * nEv * RB + i];
      c.re += p.re;
      c.im += p.im;
    }
    C[(int64_t)n * nVec + r0 + r] = c;
  }
  D[i] = Cplx<double>{c.re * invSigma[n], c.im * invSigma[n]};
}

// dst_r[k] -= sum_n v_n[k] D[n][r] for the elements k of 4 segments per workgroup, one per lane
template <typename FV, typename FS, int RB>
__global__ __launch_bounds__(256) void deflate_update_kernel(const void *const *V, void *const *Dst, int nEv, int nR, DeflateGeom g,
                                                             const Cplx<double> *D) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), e = threadIdx.x & 63;
  if (s >= g.nSeg) return;
  int64_t off;
  int valid, plane;
  seg_place(g, s, &off, &valid, &plane);
  if (e >= valid) return;
  const int64_t k = off + e;
  const auto *Vc = as_constant(V);
  const auto *Dstc = as_constant(Dst);
  Cplx<double> acc[RB];
#pragma unroll
  for (int r = 0; r < RB; r++) acc[r] = Cplx<double>{0.0, 0.0};
  constexpr int P = 4;  // eigenvectors per step; the next step's loads are issued before this step's arithmetic
  Cplx<FV> cur[P], nxt[P];
  int n = 0;
  if (nEv >= P) {
#pragma unroll
    for (int p = 0; p < P; p++) cur[p] = ld_global<FV>(Vc[p], k);
  }
  for (; n + P <= nEv; n += P) {
    const bool more = n + 2 * P <= nEv;
    if (more) {
#pragma unroll
      for (int p = 0; p < P; p++) nxt[p] = ld_global<FV>(Vc[n + P + p], k);
    }
#pragma unroll
    for (int p = 0; p < P; p++) {
      const Cplx<double> v{(double)cur[p].re, (double)cur[p].im};
#pragma unroll
      for (int r = 0; r < RB; r++) {
        const Cplx<double> d = ld_constant<double>(D, (n + p) * RB + r);
        cmadd(acc[r], v, d);
      }
    }
    if (more) {
#pragma unroll
      for (int p = 0; p < P; p++) cur[p] = nxt[p];
    }
  }
  for (; n < nEv; n++) {
    const Cplx<FV> c = ld_global<FV>(Vc[n], k);
    const Cplx<double> v{(double)c.re, (double)c.im};
#pragma unroll
    for (int r = 0; r < RB; r++) {
      const Cplx<double> d = ld_constant<double>(D, n * RB + r);
      cmadd(acc[r], v, d);
    }
  }
#pragma unroll
  for (int r = 0; r < RB; r++) {
    if (r < nR) {
      void *q = Dstc[r];
      const Cplx<FS> d = ld_global<FS>(q, k);
      st_global<FS>(q, k, (FS)((double)d.re - acc[r].re), (FS)((double)d.im - acc[r].im));
    }
  }
}

template <typename FV, typename FS, int RB>
void launch_overlap(const void *const *V, const void *const *S, int nEv, int nR, const DeflateGeom &g, int nNB, int nChunks, int segsPerChunk,
                    int gamma5, Cplx<double> *partial, hipStream_t stream) {
  hipLaunchKernelGGL((deflate_overlap_kernel<FV, FS, RB>), dim3(nNB * nChunks), dim3(256), 0, stream, V, S, nEv, nR, g, nNB, segsPerChunk,
                     gamma5, partial);
}
template <typename FV, typename FS, int RB>
void launch_update(const void *const *V, void *const *Dst, int nEv, int nR, const DeflateGeom &g, const Cplx<double> *D, hipStream_t stream) {
  hipLaunchKernelGGL((deflate_update_kernel<FV, FS, RB>), dim3((g.nSeg + 3) / 4), dim3(256), 0, stream, V, Dst, nEv, nR, g, D);
}

template <typename FV, typename FS>
void launch_pass(bool update, int RB, const void *const *V, const void *const *S, void *const *Dst, int nEv, int nR, const DeflateGeom &g,
                 int nNB, int nChunks, int segsPerChunk, int gamma5, Cplx<double> *partial, const Cplx<double> *D, hipStream_t stream) {
#define MUGIQ_DEFLATE_RB(R_)                                                                                                \
  case R_:                                                                                                                  \
    if (update) launch_update<FV, FS, R_>(V, Dst, nEv, nR, g, D, stream);                                                   \
    else launch_overlap<FV, FS, R_>(V, S, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, stream);                \
    return;
  switch (RB) {
    MUGIQ_DEFLATE_RB(4)
    MUGIQ_DEFLATE_RB(8)
    MUGIQ_DEFLATE_RB(12)
    default: break;
  }
  if (update) launch_update<FV, FS, 16>(V, Dst, nEv, nR, g, D, stream);
  else launch_overlap<FV, FS, 16>(V, S, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, stream);
#undef MUGIQ_DEFLATE_RB
}

void launch_any(int precV, int precS, bool update, int RB, const void *const *V, const void *const *S, void *const *Dst, int nEv, int nR,
                const DeflateGeom &g, int nNB, int nChunks, int segsPerChunk, int gamma5, Cplx<double> *partial, const Cplx<double> *D,
                hipStream_t stream) {
  if (precV == 8 && precS == 8) launch_pass<double, double>(update, RB, V, S, Dst, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, D, stream);
  else if (precV == 8) launch_pass<double, float>(update, RB, V, S, Dst, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, D, stream);
  else if (precS == 8) launch_pass<float, double>(update, RB, V, S, Dst, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, D, stream);
  else launch_pass<float, float>(update, RB, V, S, Dst, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5, partial, D, stream);
}

bool same_layout(const MugiqHipSpinorField &a, const MugiqHipSpinorField &b) {
  return a.field_order == b.field_order && a.volumeCB == b.volumeCB && a.stride == b.stride && a.parity_offset == b.parity_offset &&
         a.X[0] == b.X[0] && a.X[1] == b.X[1] && a.X[2] == b.X[2] && a.X[3] == b.X[3];
}

}  // namespace

int sum_over_ranks(const MugiqHipComm *comm, std::vector<double> &c) {
  // the order of the momentum projection (loop_driver.cpp): reduce over space, gather over time, fixed-order sum on the root, bcast
  const size_t n = c.size();
  std::vector<double> space(n, 0.0), gathered(n * (size_t)comm->grid[3], 0.0), sum(n, 0.0);
  int st;
  if ((st = comm->reduce_space(comm->ctx, c.data(), space.data(), n, 8)))
    return set_error(MUGIQ_HIP_ERROR_HIP, "deflateLowModes: reduce_space callback failed with status %d", st);
  if ((st = comm->gather_time(comm->ctx, space.data(), gathered.data(), n, 8)))
    return set_error(MUGIQ_HIP_ERROR_HIP, "deflateLowModes: gather_time callback failed with status %d", st);
  for (int t = 0; t < comm->grid[3]; t++)
    for (size_t i = 0; i < n; i++) sum[i] += gathered[(size_t)t * n + i];
  if ((st = comm->bcast(comm->ctx, sum.data(), n, 8)))
    return set_error(MUGIQ_HIP_ERROR_HIP, "deflateLowModes: bcast callback failed with status %d", st);
  c.swap(sum);
  return MUGIQ_HIP_SUCCESS;
}

int deflate_low_modes(const MugiqHipSpinorField *dst, const MugiqHipSpinorField *src, int nVec, const MugiqHipSpinorField *ev,
                      const double *sigma, int nEv, int gamma5, double *overlaps_h, const MugiqHipComm *comm, hipStream_t stream,
                      const char *who) {
  // ---- validation, before any device work
  MUGIQ_REQUIRE(dst != nullptr && src != nullptr && ev != nullptr, "%s: NULL argument", who);
  MUGIQ_REQUIRE(nVec >= 1, "%s: nVec = %d must be >= 1", who, nVec);
  MUGIQ_REQUIRE(nEv >= 1, "%s: nEv = %d must be >= 1", who, nEv);
  int st;
  for (int n = 0; n < nEv; n++) {
    if ((st = validate_spinor(&ev[n], who, "eVecs"))) return st;
    MUGIQ_REQUIRE(same_geometry(ev[n], ev[0]), "%s: eigenvector %d differs in precision, field order or geometry from eigenvector 0", who, n);
    MUGIQ_REQUIRE(sigma == nullptr || sigma[n] != 0.0, "%s: sigma[%d] is zero", who, n);
  }
  for (int r = 0; r < nVec; r++) {
    if ((st = validate_spinor(&src[r], who, "src"))) return st;
    if ((st = validate_spinor(&dst[r], who, "dst"))) return st;
    MUGIQ_REQUIRE(same_geometry(src[r], src[0]) && same_geometry(dst[r], src[0]),
                  "%s: src / dst vector %d differs in precision, field order or geometry from src vector 0", who, r);
  }
  MUGIQ_REQUIRE(same_layout(src[0], ev[0]), "%s: src / dst and the eigenvectors differ in field order, geometry, stride or parity offset",
                who);
  if ((st = check_disjoint(dst, nVec, "dst", src, nVec, "src", who, true, " without being identical to it"))) return st;
  const bool multi = comm != nullptr && comm->size > 1;
  if (comm) {
    MUGIQ_REQUIRE(comm->size >= 1 && comm->grid[3] >= 1, "%s: invalid comm (size %d)", who, comm->size);
    MUGIQ_REQUIRE(!multi || (comm->reduce_space && comm->gather_time && comm->bcast), "%s: a comm callback is NULL", who);
  }

  // ---- setup
  if ((st = debug_poison_lds_if_asked(stream))) return st;
  DeflateGeom g;
  g.parity_offset = ev[0].parity_offset;
  g.stride = ev[0].stride;
  g.volumeCB = ev[0].volumeCB;
  g.cpp = ev[0].field_order == 2 ? 1 : 2;
  g.planes = 12 / g.cpp;
  g.segsPerPlane = (g.cpp * g.volumeCB + kSeg - 1) / kSeg;
  g.nSeg = 2 * g.planes * g.segsPerPlane;
  const int nNB = (nEv + kNB - 1) / kNB;
  const int nChunks = std::max(1, std::min(g.nSeg, (4096 + nNB - 1) / nNB));  // about 16 workgroups per CU in pass 1
  const int segsPerChunk = (g.nSeg + nChunks - 1) / nChunks;
  const int nBlocks = (nVec + kRBMax - 1) / kRBMax;

  // device tables: [eigenvector pointers][src pointers][dst pointers][1/sigma]
  const size_t pv = sizeof(void *) * (size_t)nEv, ps = sizeof(void *) * (size_t)nVec;
  std::vector<unsigned char> host(pv + 2 * ps + sizeof(double) * (size_t)nEv);
  const void **hv = reinterpret_cast<const void **>(host.data());
  const void **hs = reinterpret_cast<const void **>(host.data() + pv);
  void **hd = reinterpret_cast<void **>(host.data() + pv + ps);
  double *hi = reinterpret_cast<double *>(host.data() + pv + 2 * ps);
  for (int n = 0; n < nEv; n++) {
    hv[n] = ev[n].data;
    hi[n] = sigma ? 1.0 / sigma[n] : 1.0;
  }
  for (int r = 0; r < nVec; r++) {
    hs[r] = src[r].data;
    hd[r] = dst[r].data;
  }
  // workspace: [partial: nChunks][nEv][16] | C: [nEv][nVec] | D: [block][nEv][16]
  const size_t partialN = (size_t)nChunks * nEv * kRBMax, cN = (size_t)nEv * nVec, dN = (size_t)nBlocks * nEv * kRBMax;
  void *ws = nullptr;
  if ((st = stream_workspace(&ws, sizeof(Cplx<double>) * (partialN + cN + dN), stream))) return st;
  void *tab = nullptr;
  if ((st = upload_table(&tab, host.data(), host.size(), stream))) return st;
  Cplx<double> *partial = static_cast<Cplx<double> *>(ws), *C = partial + partialN, *D = C + cN;
  const void *const *V_d = static_cast<const void *const *>(tab);
  const void *const *S_d = reinterpret_cast<const void *const *>(static_cast<unsigned char *>(tab) + pv);
  void *const *Dst_d = reinterpret_cast<void *const *>(static_cast<unsigned char *>(tab) + pv + ps);
  const double *inv_d = reinterpret_cast<const double *>(static_cast<unsigned char *>(tab) + pv + 2 * ps);
  const int precV = ev[0].precision, precS = src[0].precision;

  // ---- pass 1 for every block of right-hand sides (all of src is read before any dst is written: src may alias dst)
  for (int b = 0; b < nBlocks; b++) {
    const int r0 = b * kRBMax, nR = std::min(kRBMax, nVec - r0), RB = (nR + 3) / 4 * 4;
    launch_any(precV, precS, false, RB, V_d, S_d + r0, nullptr, nEv, nR, g, nNB, nChunks, segsPerChunk, gamma5 ? 1 : 0, partial, nullptr, stream);
    MUGIQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(deflate_reduce_kernel, dim3((nEv * RB + 255) / 256), dim3(256), 0, stream, partial, nChunks, nEv, RB, nR, r0, nVec,
                       inv_d, C, D + (size_t)b * nEv * kRBMax);
    MUGIQ_CHECK_HIP(hipGetLastError());
  }
  // ---- global overlaps: one synchronisation when they leave the device
  if (multi || overlaps_h) {
    std::vector<double> c(2 * cN);
    MUGIQ_CHECK_HIP(hipMemcpyAsync(c.data(), C, sizeof(Cplx<double>) * cN, hipMemcpyDeviceToHost, stream));
    MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));
    if (multi) {
      if ((st = sum_over_ranks(comm, c))) return st;
      std::vector<double> d(2 * dN, 0.0);
      for (int b = 0; b < nBlocks; b++) {
        const int r0 = b * kRBMax, nR = std::min(kRBMax, nVec - r0), RB = (nR + 3) / 4 * 4;
        for (int n = 0; n < nEv; n++)
          for (int r = 0; r < nR; r++) {
            const size_t i = ((size_t)b * nEv * kRBMax + (size_t)n * RB + r) * 2, j = ((size_t)n * nVec + r0 + r) * 2;
            d[i] = c[j] * hi[n];
            d[i + 1] = c[j + 1] * hi[n];
          }
      }
      MUGIQ_CHECK_HIP(hipMemcpyAsync(D, d.data(), sizeof(Cplx<double>) * dN, hipMemcpyHostToDevice, stream));
      MUGIQ_CHECK_HIP(hipStreamSynchronize(stream));  // d is pageable and goes out of scope
    }
    if (overlaps_h) std::copy(c.begin(), c.end(), overlaps_h);
  }
  // ---- pass 2
  for (int b = 0; b < nBlocks; b++) {
    const int r0 = b * kRBMax, nR = std::min(kRBMax, nVec - r0), RB = (nR + 3) / 4 * 4;
    launch_any(precV, precS, true, RB, V_d, nullptr, Dst_d + r0, nEv, nR, g, nNB, nChunks, segsPerChunk, 0, nullptr,
               D + (size_t)b * nEv * kRBMax, stream);
    MUGIQ_CHECK_HIP(hipGetLastError());
  }
  return MUGIQ_HIP_SUCCESS;
}

}  // namespace mugiq

extern "C" {

int mugiq_hip_deflate_low_modes(const MugiqHipSpinorField *dst_h, const MugiqHipSpinorField *src_h, int nVec,
                                const MugiqHipSpinorField *eVecs_h, const double *sigma_h, int nEv, int gamma5, double *overlaps_h,
                                const MugiqHipComm *comm, void *stream) {
  return mugiq::deflate_low_modes(dst_h, src_h, nVec, eVecs_h, sigma_h, nEv, gamma5, overlaps_h, comm, static_cast<hipStream_t>(stream),
                                  "deflateLowModes");
}

}  // extern "C"
