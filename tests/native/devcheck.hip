// Test-only device library (tests/native/libedc_devcheck.so, built by csrc/Makefile): runs the
// device builds of the field and point arithmetic headers on chosen limb inputs so that
// tests/test_gpu_device_math.py can compare them with Python integers. Not part of the product
// ABI; includes only the csrc headers and links nothing of libedc.so.
//
// Field elements travel as nine raw uint32 limbs (radix 2^29, any limb form the caller picks),
// points as 36 words X | Y | Z | T. Launch geometry is the product's: 256-thread blocks; the
// rf kernels pack four cases (one per 16-lane row) into a wave, the quad kernels sixteen, the
// row-point kernels give each of a block's four waves its own case. Buffers are padded with zeros
// to whole blocks, so the slots past ncase compute on zeros and write nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fe25519.h"
#include "ge25519.h"
#include "ge_quad.h"
#include "ge_row.h"

using namespace edc;

namespace {

enum : int {
  // fe: one lane per case
  OP_FE_MUL = 0, OP_FE_SQR, OP_FE_SUB, OP_FE_LSUB_MUL, OP_FE_MUL_LSUB, OP_FE_ADD_C, OP_FE_CARRY,
  OP_FE_MUL_SMALL, OP_FE_CANON, OP_FE_INVERT, OP_FE_POW_P58, OP_FE_FLAGS,
  // rf: one 16-lane row per case
  OP_RF_MUL = 20, OP_RF_SQR, OP_RF_SUB, OP_RF_ADD_C, OP_RF_CARRY,
  // row points: one wave per case
  OP_ROW_DBL_K = 30, OP_ROW_ADD, OP_ROW_HORNER,
  // quad points: one quad per case
  OP_QUAD_DBL = 40, OP_QUAD_ADD_CACHED, OP_QUAD_MADD, OP_QUAD_ADD, OP_QUAD_DBL_D, OP_QUAD_ADD_D,
  // lane points: one lane per case
  OP_GE_MADD_POS = 50, OP_GE_MADD_NEG, OP_GE_DBL_T, OP_GE_DBL_NOT, OP_GE_ADD_CACHED,
};

constexpr int DC_EARG = -100000;   // argument error (below every negated hipError_t)
constexpr uint32_t DC_MAX_CASES = 1u << 16;
constexpr uint32_t DC_MAX_CHAIN = 16;
constexpr int BLOCK = 256;

__device__ __forceinline__ fe dc_ld_fe(const uint32_t* p) {
  fe r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.v[i] = p[i];
  return r;
}
__device__ __forceinline__ void dc_st_fe(uint32_t* p, const fe& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) p[i] = a.v[i];
}
__device__ __forceinline__ ge_p3 dc_ld_ext(const uint32_t* p) {
  ge_p3 r;
  r.X = dc_ld_fe(p); r.Y = dc_ld_fe(p + 9); r.Z = dc_ld_fe(p + 18); r.T = dc_ld_fe(p + 27);
  return r;
}
__device__ __forceinline__ void dc_st_ext(uint32_t* p, const ge_p3& a) {
  dc_st_fe(p, a.X); dc_st_fe(p + 9, a.Y); dc_st_fe(p + 18, a.Z); dc_st_fe(p + 27, a.T);
}

// ---- fe: case = global lane ----
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_fe(uint32_t ncase, const uint32_t* __restrict__ in, uint32_t iw,
                                              uint32_t* __restrict__ out, uint32_t ow) {
  const uint32_t cs = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t* p = in + (size_t)cs * iw;
  const fe a = dc_ld_fe(p);
  fe r = fe_zero();
  uint32_t flags = 0;
  if (OP == OP_FE_MUL) r = fe_mul(a, dc_ld_fe(p + 9));
  if (OP == OP_FE_SQR) r = fe_sqr(a);
  if (OP == OP_FE_SUB) r = fe_sub(a, dc_ld_fe(p + 9));
  if (OP == OP_FE_LSUB_MUL) r = fe_mul(fe_sub_lazy(a, dc_ld_fe(p + 9)), dc_ld_fe(p + 18));
  if (OP == OP_FE_MUL_LSUB) r = fe_mul(dc_ld_fe(p + 18), fe_sub_lazy(a, dc_ld_fe(p + 9)));
  if (OP == OP_FE_ADD_C) r = fe_add_c(a, dc_ld_fe(p + 9));
  if (OP == OP_FE_CARRY) r = fe_carry(a);
  if (OP == OP_FE_MUL_SMALL) r = fe_mul_small(a, p[9]);
  if (OP == OP_FE_CANON) r = fe_canon(a);
  if (OP == OP_FE_INVERT) r = fe_invert(a);
  if (OP == OP_FE_POW_P58) r = fe_pow_p58(a);
  if (OP == OP_FE_FLAGS)
    flags = (uint32_t)fe_is_zero(a) | ((uint32_t)fe_is_negative(a) << 1) | ((uint32_t)fe_eq(a, dc_ld_fe(p + 9)) << 2);
  if (cs >= ncase) return;
  if (OP == OP_FE_FLAGS) out[(size_t)cs * ow] = flags;
  else dc_st_fe(out + (size_t)cs * ow, r);
}

// ---- rf: case = global 16-lane row, four different cases per wave ----
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_rf(uint32_t ncase, const uint32_t* __restrict__ in, uint32_t iw,
                                              uint32_t* __restrict__ out, uint32_t ow) {
  const RowCtx c = row_ctx();
  const uint32_t cs = blockIdx.x * (BLOCK / 16) + (threadIdx.x >> 4);
  const uint32_t* p = in + (size_t)cs * iw;
  const uint32_t a = c.live ? p[c.j] : 0u;
  const uint32_t b = (c.live && OP != OP_RF_SQR && OP != OP_RF_CARRY) ? p[9 + c.j] : 0u;
  uint32_t r = 0;
  if (OP == OP_RF_MUL) r = rf_mul(c, a, b);
  if (OP == OP_RF_SQR) r = rf_sqr(c, a);
  if (OP == OP_RF_SUB) r = rf_sub(c, a, b);
  if (OP == OP_RF_ADD_C) r = rf_add_c(c, a, b);
  if (OP == OP_RF_CARRY) r = rf_carry(c, a);
  if (cs < ncase) out[(size_t)cs * ow + c.j] = r;   // all 16 lanes: the padding lanes must return 0
}

// ---- row points: case = global wave, a block's four waves hold four cases ----
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_row(uint32_t ncase, const uint32_t* __restrict__ in, uint32_t iw,
                                               uint32_t* __restrict__ out, uint32_t ow) {
  const RowCtx c = row_ctx();
  const uint32_t cs = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
  const uint32_t* p = in + (size_t)cs * iw;
  uint32_t* o = out + (size_t)cs * ow;
  uint32_t x = row_ld_ext(c, p);
  if (OP == OP_ROW_DBL_K) {
    const uint32_t k = min(p[36], DC_MAX_CHAIN);
    for (uint32_t i = 0; i < k; ++i) x = row_dbl(c, x);
  } else {
    const uint32_t bq = row_cached(c, p + 36, row_d2(c));
    if (OP == OP_ROW_HORNER) {
      const uint32_t k = min(p[72], DC_MAX_CHAIN);
      for (uint32_t i = 0; i < k; ++i) x = row_dbl(c, x);
    }
    x = row_add(c, x, bq);
    if (OP == OP_ROW_ADD && cs < ncase) o[36 + (threadIdx.x & 63u)] = bq;
  }
  if (cs < ncase) row_st_ext(c, o, x);
}

// ---- quad points: case = global quad, sixteen cases per wave; every lane writes its copy ----
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_quad(uint32_t ncase, const uint32_t* __restrict__ in, uint32_t iw,
                                                uint32_t* __restrict__ out, uint32_t ow) {
  const uint32_t cs = blockIdx.x * (BLOCK / 4) + (threadIdx.x >> 2);
  const uint32_t* p = in + (size_t)cs * iw;
  const ge_p3 P = dc_ld_ext(p);
  ge_p3 r;
  if (OP == OP_QUAD_DBL) r = quad_dbl(P);
  if (OP == OP_QUAD_ADD_CACHED) r = quad_add_cached(P, ge_to_cached(dc_ld_ext(p + 36)));
  if (OP == OP_QUAD_MADD) r = quad_madd(P, ge_to_niels_affine(dc_ld_ext(p + 36)));
  if (OP == OP_QUAD_ADD) r = quad_add(P, dc_ld_ext(p + 36));
  if (OP == OP_QUAD_DBL_D) r = quad_collect(quad_dbl_d(quad_distribute(P)));
  if (OP == OP_QUAD_ADD_D) r = quad_collect(quad_add_d(quad_distribute(P), dc_ld_ext(p + 36)));
  if (cs < ncase) dc_st_ext(out + (size_t)cs * ow + 36u * (threadIdx.x & 3u), r);
}

// ---- lane points: case = global lane ----
template <int OP>
__global__ void __launch_bounds__(BLOCK) k_ge(uint32_t ncase, const uint32_t* __restrict__ in, uint32_t iw,
                                              uint32_t* __restrict__ out, uint32_t ow) {
  const uint32_t cs = blockIdx.x * BLOCK + threadIdx.x;
  const uint32_t* p = in + (size_t)cs * iw;
  const ge_p3 P = dc_ld_ext(p);
  ge_p3 r;
  if (OP == OP_GE_MADD_POS) r = ge_madd_sgn(P, ge_to_niels_affine(dc_ld_ext(p + 36)), false);
  if (OP == OP_GE_MADD_NEG) r = ge_madd_sgn(P, ge_to_niels_affine(dc_ld_ext(p + 36)), true);
  if (OP == OP_GE_DBL_T) r = ge_dbl(P, true);
  if (OP == OP_GE_DBL_NOT) r = ge_dbl(P, false);
  if (OP == OP_GE_ADD_CACHED) r = ge_add_cached(P, ge_to_cached(dc_ld_ext(p + 36)));
  if (cs < ncase) dc_st_ext(out + (size_t)cs * ow, r);
}

typedef void (*kern_t)(uint32_t, const uint32_t*, uint32_t, uint32_t*, uint32_t);

struct OpInfo {
  kern_t fn;
  uint32_t lanes, iw, ow;   // lanes per case, words in / out per case
};

#define DC_OP(K, OP, LANES, IW, OW) case OP: *o = OpInfo{K<OP>, LANES, IW, OW}; return true

bool op_info(int op, OpInfo* o) {
  switch (op) {
    DC_OP(k_fe, OP_FE_MUL, 1, 18, 9);
    DC_OP(k_fe, OP_FE_SQR, 1, 9, 9);
    DC_OP(k_fe, OP_FE_SUB, 1, 18, 9);
    DC_OP(k_fe, OP_FE_LSUB_MUL, 1, 27, 9);
    DC_OP(k_fe, OP_FE_MUL_LSUB, 1, 27, 9);
    DC_OP(k_fe, OP_FE_ADD_C, 1, 18, 9);
    DC_OP(k_fe, OP_FE_CARRY, 1, 9, 9);
    DC_OP(k_fe, OP_FE_MUL_SMALL, 1, 10, 9);
    DC_OP(k_fe, OP_FE_CANON, 1, 9, 9);
    DC_OP(k_fe, OP_FE_INVERT, 1, 9, 9);
    DC_OP(k_fe, OP_FE_POW_P58, 1, 9, 9);
    DC_OP(k_fe, OP_FE_FLAGS, 1, 18, 1);
    DC_OP(k_rf, OP_RF_MUL, 16, 18, 16);
    DC_OP(k_rf, OP_RF_SQR, 16, 9, 16);
    DC_OP(k_rf, OP_RF_SUB, 16, 18, 16);
    DC_OP(k_rf, OP_RF_ADD_C, 16, 18, 16);
    DC_OP(k_rf, OP_RF_CARRY, 16, 9, 16);
    DC_OP(k_row, OP_ROW_DBL_K, 64, 37, 36);
    DC_OP(k_row, OP_ROW_ADD, 64, 72, 100);
    DC_OP(k_row, OP_ROW_HORNER, 64, 73, 36);
    DC_OP(k_quad, OP_QUAD_DBL, 4, 36, 144);
    DC_OP(k_quad, OP_QUAD_ADD_CACHED, 4, 72, 144);
    DC_OP(k_quad, OP_QUAD_MADD, 4, 72, 144);
    DC_OP(k_quad, OP_QUAD_ADD, 4, 72, 144);
    DC_OP(k_quad, OP_QUAD_DBL_D, 4, 36, 144);
    DC_OP(k_quad, OP_QUAD_ADD_D, 4, 72, 144);
    DC_OP(k_ge, OP_GE_MADD_POS, 1, 72, 36);
    DC_OP(k_ge, OP_GE_MADD_NEG, 1, 72, 36);
    DC_OP(k_ge, OP_GE_DBL_T, 1, 36, 36);
    DC_OP(k_ge, OP_GE_DBL_NOT, 1, 36, 36);
    DC_OP(k_ge, OP_GE_ADD_CACHED, 1, 72, 36);
    default: return false;
  }
}

}  // namespace

// Runs op on ncase cases: in / out are HOST pointers (ncase * words_per_case words each). Returns
// 0, the negated hipError_t, or DC_EARG (unknown op, ncase > 2^16, word counts that do not match
// the op, a null buffer) without launching anything.
extern "C" __attribute__((visibility("default")))
int dc_run(int op, uint32_t ncase, const uint32_t* in, uint32_t in_words_per_case,
           uint32_t* out, uint32_t out_words_per_case) {
  OpInfo oi;
  if (!op_info(op, &oi)) return DC_EARG;
  if (ncase > DC_MAX_CASES || in_words_per_case != oi.iw || out_words_per_case != oi.ow) return DC_EARG;
  if (ncase == 0) return 0;
  if (!in || !out) return DC_EARG;
  const uint32_t per_block = BLOCK / oi.lanes;
  const uint32_t nblk = (ncase + per_block - 1) / per_block;
  const size_t slots = (size_t)nblk * per_block;            // whole blocks: the tail slots read zeros
  const size_t in_bytes = slots * oi.iw * sizeof(uint32_t), out_bytes = slots * oi.ow * sizeof(uint32_t);
  uint32_t *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_in, in_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, out_bytes);
  if (e == hipSuccess) e = hipMemset(d_in, 0, in_bytes);
  if (e == hipSuccess) e = hipMemset(d_out, 0, out_bytes);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, (size_t)ncase * oi.iw * sizeof(uint32_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(oi.fn, dim3(nblk), dim3(BLOCK), 0, 0, ncase, (const uint32_t*)d_in, oi.iw, d_out, oi.ow);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)ncase * oi.ow * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return e == hipSuccess ? 0 : -(int)e;
}
