// The two-sided matrix-pipe tile (csrc/fused_mfma_kernel.h, TWO) for fp64 FLOAT2 eigenvectors: every column tile but TJ = 12, both row tiles.
#include "fused_mfma_kernel.h"

namespace mugiq {
int launch_mfma_tile_two_d2(const MTileArgs &a, int dir, int sign, int ns, const MfmaLaunch &g, hipStream_t stream) {
  return launch_mfma_tile_t<double, 2, true, true>(a, dir, sign, ns, g, stream);
}
}  // namespace mugiq
