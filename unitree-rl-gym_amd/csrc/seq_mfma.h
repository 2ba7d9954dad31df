// seq_mfma.h — what lstm_seq.hip, gru_seq.hip and heads.hip share: the shape of the matrix-core
// sequence kernels, the bf16 and accumulator vector types, the split of an fp32 value into bf16
// hi + lo, the fast activations, the partner-lane exchange, and the host side's error text,
// launch status and step-tile rule.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

// the hidden-64 memories on the matrix cores (LSTM and GRU)
constexpr int ME = 16, MH = 64, MG = 256, MKX = 64;  // envs per workgroup, hidden, saved row (4 x 64), x slots
constexpr int MLDA = MKX + MH + 8;                   // LDS row stride of [x | h] (bf16): 272 B

typedef __bf16 mbf16;
typedef mbf16 mbf16x8 __attribute__((ext_vector_type(8)));
typedef mbf16 mbf16x4 __attribute__((ext_vector_type(4)));
typedef float mfloatx4 __attribute__((ext_vector_type(4)));
typedef float mfloatx16 __attribute__((ext_vector_type(16)));

// activations of the MFMA kernels: v_exp_f32 + v_rcp_f32.  Measured on exact-grid inputs against
// fp64 (tests/test_gpu_seq_reference.py): fsig within 1.6 * 2^-24 (9.2e-8) and ftanh within
// 3.0 * 2^-24 (1.8e-7) absolute, what the same operations correctly rounded give; the budgets the
// tests hold them to are derived in tests/seq_ref.py
static __device__ __forceinline__ float fsig(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
static __device__ __forceinline__ float ftanh(float x) { return 2.f * __builtin_amdgcn_rcpf(1.f + __expf(-2.f * x)) - 1.f; }

static __device__ __forceinline__ void split_bf16(float v, mbf16& hi, mbf16& lo) {
    hi = (mbf16)v;
    lo = (mbf16)(v - (float)hi);
}

// the value of lane j ^ 8 of the same row of 16 (DPP row_ror:8, one VALU move)
static __device__ __forceinline__ float ror8(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
}

// host side, defined in lstm_seq.hip: the text behind pmlp_lstm_last_error (one for the LSTM,
// the GRU and the heads), the status after a launch, and the 16-env tiles per workgroup of a
// single rollout step
namespace pmlp_seq {
__attribute__((visibility("hidden"))) int fail(const std::string& m);
__attribute__((visibility("hidden"))) int launched(const char* what);
__attribute__((visibility("hidden"))) int step_tiles(int B);
}  // namespace pmlp_seq
