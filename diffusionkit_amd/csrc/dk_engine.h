// What the host translation units behind include/dk_hip.h share: abi_ops.hip (the stand-alone operator entries and dk_tune_set),
// mmdit_engine.hip and vae_engine.hip (the engines that sequence the gfx950 kernels).  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <unordered_map>

#include "../../include/dk_hip.h"
#include "dk_kernels.h"

// dk_tune_set knobs of the engines (the routing's own are declared in dk_kernels.h); each is defined, with its values, in the file that reads it
extern int g_dk_fuse_k, g_dk_fuse_qg, g_dk_fuse_q;  // mmdit_engine.hip
extern int g_dk_conv_halo;                          // vae_engine.hip
extern int g_dk_pitch_min_k;                        // abi_ops.hip

static inline hipStream_t S_(void* s) { return (hipStream_t)s; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define DK_TRY(expr)          \
  do {                        \
    int _rc = (expr);         \
    if (_rc != 0) return _rc; \
  } while (0)

struct Carver {
  char* base;
  size_t off, cap;
  bool dry;
  Carver(void* b, size_t c) : base((char*)b), off(0), cap(c), dry(b == nullptr) {}
  void* take(size_t bytes) {
    off = align_up(off, 256);
    void* p = dry ? nullptr : (void*)(base + off);
    off += bytes;
    return p;
  }
};

// What an entry point knows about the launches it builds and hands down to whatever builds one: plain arguments, no state outside the call.
// Two engines, on one host thread in turn or on two threads / streams at once, therefore never share an element type or a split region.  (A
// single engine must not be driven from two streams concurrently: its activations live in one workspace anyway.)
struct LaunchCtx {
  hipStream_t st;
  int dtype;            // element type of every launch: DK_DTYPE_BF16 / DK_DTYPE_F16
  void* kws = nullptr;  // the caller's K-split region (fp32 slabs + flags, dk_gemm_split_workspace_bytes()) for Linear::split_ws, or null
  AttnWs aws;           // ... and its attention key-split region for dk_launch_attention (empty: no launch is split)
};
// an elementwise launcher in element type dtype (dk_elem_launchers.h: same signature in both)
#define DK_EL(dtype, fn) ((dtype) == DK_DTYPE_F16 ? dk_f16::fn : fn)

inline int need(const std::unordered_map<std::string, const void*>& named, const std::string& name, const bf16_t** out, bool optional = false) {
  auto it = named.find(name);
  if (it == named.end()) {
    *out = nullptr;
    if (optional) return 0;
    dk_set_error("weight not bound: " + name);
    return -3;
  }
  *out = (const bf16_t*)it->second;
  return 0;
}

inline int mx_nblk(long rows) { return (int)((rows + 127) / 128 + 1); }
inline Mx8Out mx8_out(void* out, void* scales, int ldo, long rows, int row0, int seg_len, int seg_stride, int col0) {
  Mx8Out o;
  o.out = (unsigned char*)out; o.scales = (unsigned char*)scales; o.ldo = ldo; o.n_blk128 = mx_nblk(rows); o.row0 = row0;
  o.seg_len = seg_len; o.seg_stride = seg_stride; o.col0 = col0;
  return o;
}

// ---- Linear launches ------------------------------------------------------------------------------------------------------------
// The rows of a matrix as a GEMM operand addresses them (GemmParams, dk_kernels.h): logical row m is physical row
// (m / seg_len) * seg_stride + m % seg_len of a buffer of pitch ld elements.  seg_len == 0: one segment, the M rows of the launch.
struct Rows {
  bf16_t* p;
  int ld, seg_len, seg_stride;
};
inline Rows dense(const bf16_t* p, int ld) { return Rows{(bf16_t*)p, ld, 0, 0}; }  // plain [M, ld] (read-only operands come through here too)

// gate[(m / gate_seg_len) * gate_stride + n] and the residual rows of DK_EPI_GATE_RES / DK_EPI_RES (GemmParams and GemmF8Params)
template <class P>
inline void set_gate_res(P& p, const bf16_t* gate, int gate_seg_len, int gate_stride, Rows res) {
  p.gate = gate; p.gate_seg_len = gate_seg_len > 0 ? gate_seg_len : p.M; p.gate_stride = gate_stride;
  p.res = res.p; p.ldr = res.ld; p.r_seg_len = res.seg_len > 0 ? res.seg_len : p.M; p.r_seg_stride = res.seg_stride;
}

// C = epi(A @ W^T + bias) in element type dtype_: W [N, ldw >= K] (0: K).  Launch with dk_launch_gemm / dk_launch_gemm_pair.
struct Linear : GemmParams {
  Linear(int dtype_, Rows A_, const bf16_t* W_, const bf16_t* bias_, Rows C_, int M_, int N_, int K_, int epi_, int ldw_ = 0) {
    memset(static_cast<GemmParams*>(this), 0, sizeof(GemmParams));
    A = A_.p; W = W_; C = C_.p; bias = bias_;
    M = M_; N = N_; K = K_; lda = A_.ld; ldc = C_.ld; ldw = ldw_;
    a_seg_len = A_.seg_len > 0 ? A_.seg_len : M; a_seg_stride = A_.seg_stride;
    c_seg_len = C_.seg_len > 0 ? C_.seg_len : M; c_seg_stride = C_.seg_stride;
    r_seg_len = gate_seg_len = M;
    alpha = 1.0f; epi = epi_; dtype = dtype_;
  }
  Linear& gate_res(const bf16_t* gate_, int gate_seg_len_, int gate_stride_, Rows res_) {
    set_gate_res(*this, gate_, gate_seg_len_, gate_stride_, res_);
    return *this;
  }
  // with the calling engine's K-split region (LaunchCtx::kws): dk_gemm_route may then cut a launch that fills a fraction of a round of the CUs
  // along K (another summation order) -- which launches carry it is part of their results
  Linear& split_ws(void* kws) {
    if (kws) { workspace = kws; workspace_bytes = dk_gemm_split_workspace_bytes(); }
    return *this;
  }
};

// ---- abi_ops.hip, used by the engines: the typed implementations behind the exported *_bf16 / *_f16 operator entries --------------------
// workspace: optional K-split scratch (dk_gemm_split_workspace_bytes) for stages whose tiles fill only half the CUs; rec: record the route
// instead of launching (dk_conv3x3_plan)
int conv3x3_launch(int dtype, const dk_conv_desc* d, void* workspace, hipStream_t stream, dk_gemm_plan_t* rec = nullptr);
// transpose of every image's V into [512, Tp] rows (zero-padded), then the flash kernel
int attention_d512(int dtype, const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int T, int ld, int ldo, float scale,
                   bf16_t* vt, hipStream_t st);
// scratch layout shared by the two: [partials: B * n * 2G][mean_rstd: B * G * 2], n = the larger of 1024 and the caller's n_partial
int groupnorm_launch(int dtype, const void* x, void* y, int B, long HW, int C, int G, const void* gamma, const void* beta, float eps,
                     int fuse_silu, float* scratch, hipStream_t st);
int groupnorm_table_launch(int dtype, const void* x, int B, long HW, int C, int G, const void* gamma, const void* beta, float eps,
                           float* scratch, int n_partial, float* scale_shift, hipStream_t st);
