// secp256k1 batch multiply with the field multiply INLINED into the group-law routines (no call, no
// argument marshalling through v0..v17; the doubling loop stays rolled so the window body fits the
// instruction cache).  mul_var_batch (mulvar.hip) takes it whenever it has scratch; its other
// kernels use the out-of-line multiply.  The curve twin CurveSecpI (curves.hpp) gives the kernels their own names -
// both translation units ship their own code object - and selects the fused ladder formulas.
#define NCG_MUL_INLINE 1
#include "mulvar_pairsum.hpp"
#include "host_api.hpp"

namespace ncg {

hipError_t mul_var_secp_inline(const uint32_t* pts, const uint32_t* scalars, uint32_t* out, uint8_t* out_inf, int n,
                               uint32_t* jac_tmp, hipStream_t st) {
  // large batches: one addition per window from affine pair sums (mulvar_pairsum.hpp); its two extra launches do not pay below
  if (n >= PAIRSUM_MIN_N) return launch_mul_var_pairsum<CurveSecpI, 4, 3, 16>(pts, scalars, out, out_inf, n, jac_tmp, st);
  return launch_mul_var_gtab<CurveSecpI, 4, 3, 16>(pts, scalars, out, out_inf, n, jac_tmp, st);  // W = 4, 3 waves/SIMD
}

}  // namespace ncg
