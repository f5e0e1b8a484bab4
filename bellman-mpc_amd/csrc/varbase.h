// Host interface of the per-element variable-base scalar multiplication (varbase.hip) that the
// ceremony rounds (mpc.cpp) are built on.  Every function enqueues on ctx->stream and returns
// synchronised; the caller holds ctx->mu and has set the device.
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

namespace bh {
// canonical scalars, 4 LE u64
inline bool scalar_below_r(const uint64_t w[4]) { return !geq_p<4>(w); }
inline bool scalar_is_zero(const uint64_t w[4]) { return !(w[0] | w[1] | w[2] | w[3]); }
inline int scalar_bits(const uint64_t w[4]) {
  for (int k = 3; k >= 0; k--)
    if (w[k]) return 64 * k + 64 - __builtin_clzll(w[k]);
  return 0;
}

void varbase_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// out[i] = k_i * in[i].  d_sc: canonical scalars (8 LE u32 each) below 2^nbits (1..255) and below r, read
// with a stride of 8 words (per element) or 0 (d_sc[0] for every element).
// BH_ERR_UNEXPECTED_IDENTITY: an identity in `in`, or a scalar that is zero (found on the device
// before the normalisation, which a zero ZZ would poison).
bh_status varbase_mul(bh_ctx* ctx, const bh_srs* in, const uint32_t* d_sc, int stride, int nbits, bh_srs* out);
// One chunk of that multiplication enqueued on st, for callers that go on with the products
// unnormalised (group_fft.hip): d_xyzz[i] = k_i * d_pts[i], i < k, as XYZZ.  W windows, the top one
// biased or not as k_varbase_mul_win takes them (255-bit scalars: W = 64, top_biased = 1).  A
// product that is the identity is stored as the all-zero point and raises *d_flag.  Workspace:
// d_xyzz 8 k points, d_scr 8 k field elements + 64 B, d_table 8 k packed records.
template <class C>
hipError_t varbase_mul_chunk(const uint32_t* d_pts, const uint32_t* d_sc, int stride, size_t k, int W, int top_biased,
                             void* d_xyzz, void* d_scr, uint32_t* d_table, uint32_t* d_flag, hipStream_t st);
// The table that multiplication reads, alone: 1P .. 8P of the k points of d_pts as packed affine
// records, digit-major (record d k + i holds (d + 1) P_i), enqueued on st.  No point may be the
// identity or of order <= 8.  Workspace as above.
template <class C>
hipError_t varbase_multiples_table(const uint32_t* d_pts, size_t k, void* d_xyzz, void* d_scr, uint32_t* d_table,
                                   hipStream_t st);
constexpr size_t VB_WIN_CHUNK = (size_t)1 << 18;  // points per chunk of the windowed multiplication
// out[i] = in[lo2 + i] - in[lo1 + i], i < n; a difference that is the identity:
// BH_ERR_UNEXPECTED_IDENTITY
bh_status varbase_sub(bh_ctx* ctx, const bh_srs* in, size_t lo1, size_t lo2, size_t n, bh_srs* out);
// d_sc[i] = (a x^i)^(+-1), i < n, canonical; a or x zero: BH_ERR_UNEXPECTED_IDENTITY, >= r:
// BH_ERR_INVALID_ARGUMENT
bh_status varbase_power_scalars(bh_ctx* ctx, size_t n, const uint64_t a[4], const uint64_t x[4], int invert,
                                DevBuf* d_sc);
// `count` host scalars (4 LE u64 each) checked (< r, < 2^nbits: BH_ERR_INVALID_ARGUMENT) and copied
bh_status varbase_upload_scalars(bh_ctx* ctx, const uint64_t* scalars, size_t count, int nbits, DevBuf* d_sc);
}  // namespace bh
