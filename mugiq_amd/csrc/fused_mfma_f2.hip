// The matrix-pipe tile (csrc/fused_mfma_kernel.h) for fp32 FLOAT2 eigenvectors: 16-line column tiles, 8-wave row tile.
#include "fused_mfma_kernel.h"

namespace mugiq {
int launch_mfma_tile_f2(const MTileArgs &a, int dir, int sign, int ns, const MfmaLaunch &g, hipStream_t stream) {
  return launch_mfma_tile_t<float, 2, false>(a, dir, sign, ns, g, stream);
}
}  // namespace mugiq
