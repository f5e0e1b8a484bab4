// Internal interface of the device-resident KeypairAssembly (r1cs.hip) and what it borrows from
// the chain generator (chain.hip) and the NTT plumbing (api.hip).
#pragma once
#include <vector>

#include "api_internal.h"
#include "kinfo.h"

// KeypairAssembly in HBM (generator.rs:44-156): the term lists of A, B and C concatenated in the
// column order [A inputs, A aux, B inputs, B aux, C inputs, C aux] (3 * (ni + na) columns), every
// column cut into segments of at most bh::R1CS_S terms.  Segments tile the term array in order, so
// seg[k] .. seg[k + 1] is segment k and colseg[j] .. colseg[j + 1] are column j's segments.
struct bh_r1cs {
  int device = 0;
  size_t ni = 0, na = 0;
  size_t nc = 0;            // constraints including the ni appended rows input_i * 0 = 0
  size_t m = 0;             // domain size of nc
  uint32_t L = 0;
  size_t nnz[3] = {0, 0, 0};  // A (with the appended terms), B, C
  size_t terms = 0, nseg = 0, ncol = 0, nlong = 0;
  bh::DevBuf coeff;         // terms x 8 u32, packed device Montgomery
  bh::DevBuf row;           // terms u32
  bh::DevBuf seg;           // nseg + 1 u32: first term of each segment, seg[nseg] = terms
  bh::DevBuf colseg;        // ncol + 1 u32: first segment of each column
  bh::DevBuf longcols;      // nlong u32: the columns with more than R1CS_S segments
  // ProvingAssignment's density maps (prover.rs:99-139): bit i = the circuit put at least one term
  // into variable i's column of A (aux) / B (inputs, aux).  A function of the column pointers alone
  // (the appended rows touch only A's input columns, which have no map), so bh_r1cs_create keeps them
  std::vector<uint64_t> a_aux_density, b_input_density, b_aux_density;
  // The row view bh_r1cs_witness multiplies with: the same terms listed by row.  Row k * m + i is
  // constraint i of matrix k (A, B, C), so the products land in a witness's a | b | c buffer as they
  // are and the rows nc .. m are empty.  Built on the device by the first bh_r1cs_witness of the
  // handle, under rv.mu, which every call holds to its end (rv.words is per-call state); a handle
  // that only generates parameters never allocates any of it.  Coefficients are not copied: a row's
  // entry is the term's index into coeff and its variable, 8 bytes per term.
  struct RowView {
    std::mutex mu;
    bool ready = false;
    size_t nrows = 0, nseg = 0, nlong = 0;
    bh::DevBuf term;      // terms u32: index into coeff / row, grouped by row
    bh::DevBuf var;       // terms u32: that term's variable (inputs, then aux)
    bh::DevBuf seg;       // nseg + 1 u32: first entry of each row segment, seg[nseg] = terms
    bh::DevBuf rowseg;    // nrows + 1 u32: first segment of each row
    bh::DevBuf longrows;  // nlong u32: the rows with more than R1CS_S segments
    bh::DevBuf words;     // 2 u32: [0] the long rows' counter (build), [1] first unsatisfied row
  };
  mutable RowView rv;
};

namespace bh {
// terms per segment = the dependent Fr products one lane of the QAP kernel runs at most
constexpr uint32_t R1CS_S = 32;

void r1cs_kernels(std::vector<KernInfo>& v);  // scratch budget (scratch.cpp)

// chain.hip: the generators and their 32 x 255 fixed-base window tables (crs.hip's layout)
Jac<Fp> crs_g1_gen();
Jac<Fp2> crs_g2_gen();
std::vector<AffinePt<Fp>> crs_table_g1();
std::vector<AffinePt<Fp2>> crs_table_g2();

// r1cs.hip: n canonical non-zero scalars on the device -> n packed affine points d_sc[i] * G through
// crs.hip's fixed_base_batch, in chunks; tab: crs_table_g1 / _g2 on the device.  Synchronises
// ctx->stream (caller holds ctx->mu)
template <class C>
bh_status fixed_base_device(bh_ctx* ctx, const bh_srs& tab, const uint32_t* d_sc, size_t n, bh_srs* out);

// r1cs.hip, for callers whose vectors are resident (params_check.hip); the caller holds ctx->mu.
// r1cs_powers_device: d_out[i] = x^i, i < n, packed device Montgomery (k_r1cs_powers), on ctx->stream,
// synchronised.  r1cs_eval_device: the QAP evaluation behind bh_r1cs_eval, u | v | w (3 (ni + na)
// values) into d_y for the m values d_x, d_part max(nseg, 1) values of scratch; enqueued on st.
// r1cs_rows_device: the row product behind bh_r1cs_witness, a | b | c = A z | B z | C z (3 m values,
// the rows nc .. m zero) for z = [inputs, aux] (packed device Montgomery, < 2r); builds the handle's
// row view on first use (under its lock), sizes *part as scratch, enqueues on st
bh_status r1cs_powers_device(bh_ctx* ctx, const Fr& x, size_t n, uint32_t* d_out);
hipError_t r1cs_eval_device(const bh_r1cs* r, const uint32_t* d_x, uint32_t* d_part, uint32_t* d_y, hipStream_t st);
bh_status r1cs_rows_device(const bh_r1cs* r, const uint32_t* d_z, DevBuf* part, uint32_t* d_abc, hipStream_t st);

// api.hip: the ifft (domain.rs:104-121) of 2^L packed device-Montgomery Fr resident in d_a, natural
// order in and out, d_tmp the same size; enqueued on ctx->stream (caller holds ctx->mu)
bh_status device_ifft(bh_ctx* ctx, Domain* D, uint32_t* d_a, uint32_t* d_tmp);
}  // namespace bh
