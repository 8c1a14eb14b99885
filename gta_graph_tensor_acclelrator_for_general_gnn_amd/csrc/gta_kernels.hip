// gta_kernels.hip -- hand-written CDNA4 (gfx950) kernels + the extern "C" ABI of
// libgta (declared in include/gta.h).  Each kernel executes one ISA op / fused
// pattern of the GTA instruction stream; see gta.h for the reference citation of
// each entry point and DESIGN.md for the HBM layout and rooflines.
//
// Wave = 64 lanes.  Workgroups are 256 threads (4 waves) everywhere.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "../../include/gta.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define GTA_HIP(x)                                                                   \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) return fail(GTA_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define GTA_LAUNCHED(name)                                                                      \
  do {                                                                                          \
    hipError_t e_ = hipGetLastError();                                                          \
    if (e_ != hipSuccess) return fail(GTA_ERR_HIP, std::string(name) + ": " + hipGetErrorString(e_)); \
  } while (0)

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
__host__ __device__ inline bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) % bytes) == 0; }

// ---------------------------------------------------------------------------
// special functions (SF post-ops) and binary ops
// ---------------------------------------------------------------------------
// Special values: gta.h, "Special values of the SFs".  NaN in gives NaN out of every SF.
__device__ __forceinline__ float sf_apply(int sf, float v) {
  switch (sf) {
    case GTA_SF_NONE: return v;
    // not v > 0 ? v : 0: NaN compares false and would become a clean 0 (np.maximum and torch.relu give
    // NaN); bitwise the same result on every other input
    case GTA_SF_RELU: return v <= 0.f ? 0.f : v;
    case GTA_SF_EXP_LEAKY_RELU: return expf(v > 0.f ? v : 0.2f * v);
    case GTA_SF_ELU: return v > 0.f ? v : expm1f(v);
    case GTA_SF_EXP: return expf(v);
    case GTA_SF_LEAKY_RELU: return v > 0.f ? v : 0.2f * v;
    // expf(-v) is inf below v = -88.72 and the quotient 0 there, where the sigmoid is still a denormal
    // (gta.h states it; DESIGN.md 3.5: taking expf(v) there costs every SF epilogue its registers)
    case GTA_SF_SIGMOID: return 1.f / (1.f + expf(-v));
    case GTA_SF_TANH: return tanhf(v);
    case GTA_SF_RECIP: return 1.f / v;
    default: return v;
  }
}

__device__ __forceinline__ float bin_apply(int bin, float a, float b) {
  switch (bin) {
    case GTA_BIN_ADD: return a + b;
    case GTA_BIN_MUL: return a * b;
    case GTA_BIN_DIV: return a / b;
    case GTA_BIN_SUB: return a - b;
    default: return a;
  }
}

// ---------------------------------------------------------------------------
// vector helpers
// ---------------------------------------------------------------------------
template <int VW> struct Vec;
template <> struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v[0]; }
};
template <> struct Vec<2> {
  float v[2];
  __device__ __forceinline__ void load(const float* p) {
    float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x; v[1] = t.y;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]); }
};
template <> struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <> struct Vec<8> {  // bf16 rows only: 8 elements = one 16-B piece (fp32 sides: two float4)
  float v[8];
  __device__ __forceinline__ void load(const float* p) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
};

// Vec<VW> from VW consecutive elements of a float or bf16 row (bf16 widened exactly: bits << 16)
template <int VW>
__device__ __forceinline__ void load_row(Vec<VW>& o, const float* p) { o.load(p); }
template <int VW>
__device__ __forceinline__ void load_row(Vec<VW>& o, const uint16_t* p) {
  if constexpr (VW == 8) {  // one 16-B load (8-B aligned rows are fine for global loads)
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    o.v[0] = __uint_as_float(u.x << 16); o.v[1] = __uint_as_float(u.x & 0xffff0000u);
    o.v[2] = __uint_as_float(u.y << 16); o.v[3] = __uint_as_float(u.y & 0xffff0000u);
    o.v[4] = __uint_as_float(u.z << 16); o.v[5] = __uint_as_float(u.z & 0xffff0000u);
    o.v[6] = __uint_as_float(u.w << 16); o.v[7] = __uint_as_float(u.w & 0xffff0000u);
  } else if constexpr (VW == 4) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    o.v[0] = __uint_as_float(u.x << 16); o.v[1] = __uint_as_float(u.x & 0xffff0000u);
    o.v[2] = __uint_as_float(u.y << 16); o.v[3] = __uint_as_float(u.y & 0xffff0000u);
  } else if constexpr (VW == 2) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
    o.v[0] = __uint_as_float(u << 16); o.v[1] = __uint_as_float(u & 0xffff0000u);
  } else {
    o.v[0] = __uint_as_float(static_cast<uint32_t>(*p) << 16);
  }
}
__device__ __forceinline__ float load_elem(const float* p) { return *p; }
__device__ __forceinline__ float load_elem(const uint16_t* p) { return __uint_as_float(static_cast<uint32_t>(*p) << 16); }
__device__ __forceinline__ uint16_t to_bf16_bits(float f) {
  return __builtin_bit_cast(uint16_t, __float2bfloat16(f));  // round to nearest even
}
__device__ __forceinline__ uint16_t to_bf16_bits(uint16_t b) { return b; }

__device__ __forceinline__ int wave_id_uniform() {
  return __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
}

// ---------------------------------------------------------------------------
// Aggregate plan (row chunks).  Layout inside the caller's plan buffer:
//   int64 hdr[8]            : n_items, n_split, chunk, max_items, n_rows
//   int32 item_row[max_items]  : the item's row, bit 31 set when the row is split over several items
//   int64 item_beg[max_items]
//   int64 item_end[max_items]  : (begin, end) of the item's edges: an item's bounds in one level of
//                                loads, no dependent indptr read (short rows: one fewer round trip)
//   int32 split_row[n_rows], int32 split_first[n_rows], int32 split_cnt[n_rows]
//   int64 offs[n_rows]      : exclusive scan of chunks per row (scratch)
// ---------------------------------------------------------------------------
struct PlanView {
  int64_t* hdr;
  int32_t* item_row;
  int64_t* item_beg;
  int64_t* item_end;
  int32_t* split_row;
  int32_t* split_first;
  int32_t* split_cnt;
  int64_t* offs;
};

inline int64_t round16(int64_t b) { return (b + 15) / 16 * 16; }
inline int64_t max_items_for(int64_t n_rows, int64_t nnz, int64_t chunk) {
  return n_rows + (nnz + chunk - 1) / chunk;
}

PlanView plan_view(void* base, int64_t n_rows, int64_t max_items) {
  char* p = static_cast<char*>(base);
  PlanView v;
  v.hdr = reinterpret_cast<int64_t*>(p); p += round16(8 * sizeof(int64_t));
  v.item_row = reinterpret_cast<int32_t*>(p); p += round16(max_items * 4);
  v.item_beg = reinterpret_cast<int64_t*>(p); p += round16(max_items * 8);
  v.item_end = reinterpret_cast<int64_t*>(p); p += round16(max_items * 8);
  v.split_row = reinterpret_cast<int32_t*>(p); p += round16(n_rows * 4);
  v.split_first = reinterpret_cast<int32_t*>(p); p += round16(n_rows * 4);
  v.split_cnt = reinterpret_cast<int32_t*>(p); p += round16(n_rows * 4);
  v.offs = reinterpret_cast<int64_t*>(p); p += round16((n_rows + 1) * 8);
  return v;
}

int64_t plan_bytes_for(int64_t n_rows, int64_t max_items) {
  return round16(8 * 8) + round16(max_items * 4) + 2 * round16(max_items * 8) + 3 * round16(n_rows * 4) +
         round16((n_rows + 1) * 8);
}

__device__ __forceinline__ int64_t chunks_of(int64_t deg, int64_t chunk) {
  return deg <= chunk ? 1 : (deg + chunk - 1) / chunk;
}

// single-workgroup exclusive scan of per-row chunk counts (plan build only)
__global__ void __launch_bounds__(1024) k_plan_scan(const int64_t* __restrict__ indptr, int64_t n_rows, int64_t chunk,
                                                     int64_t* __restrict__ offs, int64_t* __restrict__ hdr) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n_rows + 1023) / 1024;
  const int64_t b = min<int64_t>(n_rows, t * per), e = min<int64_t>(n_rows, b + per);
  int64_t s = 0;
  for (int64_t r = b; r < e; ++r) s += chunks_of(indptr[r + 1] - indptr[r], chunk);
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    int64_t v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = (t == 0) ? 0 : part[t - 1];
  for (int64_t r = b; r < e; ++r) {
    offs[r] = run;
    run += chunks_of(indptr[r + 1] - indptr[r], chunk);
  }
  if (t == 1023) {
    hdr[0] = part[1023];  // n_items
    hdr[1] = 0;           // n_split (filled by k_plan_fill)
    hdr[2] = chunk;
    hdr[3] = n_rows;
  }
}

__global__ void k_plan_fill(const int64_t* __restrict__ indptr, int64_t n_rows, int64_t chunk, PlanView v) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t b = indptr[r], deg = indptr[r + 1] - b;
  const int64_t nc = chunks_of(deg, chunk), off = v.offs[r];
  for (int64_t j = 0; j < nc; ++j) {
    v.item_row[off + j] = static_cast<int32_t>(nc > 1 ? (static_cast<uint32_t>(r) | 0x80000000u) : r);
    v.item_beg[off + j] = b + j * chunk;
    v.item_end[off + j] = min(b + (j + 1) * chunk, b + deg);
  }
  if (nc > 1) {  // compaction order is arbitrary; each split row's sum order is fixed
    unsigned long long s = atomicAdd(reinterpret_cast<unsigned long long*>(&v.hdr[1]), 1ull);
    v.split_row[s] = static_cast<int32_t>(r);
    v.split_first[s] = static_cast<int32_t>(off);
    v.split_cnt[s] = static_cast<int32_t>(nc);
  }
}

// ---------------------------------------------------------------------------
// K6/K7/K2 aggregate.
//   One wavefront per work item (a whole row, or a <=chunk slice of a long row).
//   LPE lanes cover one edge's feature slice (VW floats per lane per vector,
//   NV vectors per lane); 64/LPE edges share one wave instruction.  The edge
//   loop issues U independent row loads before consuming any (latency hiding),
//   source indices are fetched 64 at a time with one coalesced load and
//   broadcast by readlane (LPE==64: wave-uniform row base in SGPRs) or
//   ds_bpermute.  Accumulation is fp32 in VGPRs, in a fixed order: results are
//   bitwise reproducible run to run (no atomics).
// ---------------------------------------------------------------------------
enum { XM_IDX = 0, XM_EDGE = 1, XM_EX1 = 2, XM_EX2 = 3, XM_EX3 = 4 };

// XM_EX*: the gathered value of edge e is an expression of K3 apply_edge ops over up to four
// operand rows (gta_aggregate_expr; DGN's op 2-7 tree, PNA's op 5-7), evaluated as the edge is
// summed -- the [E, F] edge tensors the tree's ops would store are never written.  Per element,
// with L0..L3 the operands' values:
//   XM_EX1: t = sf0(L0 bin0 L1)             (bin0 NONE: sf0(L0))
//   XM_EX2: u = sf0(L0 bin0 L1); t = sf1(swap ? L2 bin1 u : u bin1 L2)
//   XM_EX3: u = sf0(L0 bin0 L1); v = sf1(L2 bin1 L3); t = sf2(u bin2 v)
// each step sf_apply(bin_apply()) as k_apply_edge* computes it, each intermediate an fp32 value as
// the stored edge tensor holds it (no contraction across steps), summed in k_aggregate's XM_EDGE
// order: bitwise the unfused apply_edge ops + gather.  Operand modes: GTA_IDX_EDGE (row e; ld 0:
// one row broadcast to every edge), GTA_IDX_SRC (row indices[e]), GTA_IDX_DST (the item's row).
// Every operand is loaded per edge (row-constant ones hit L1).  Each step runs
// over a whole unrolled step's values under ONE uniform switch on its op (per-element switches
// made a 6.6 k-instruction kernel 7x slower than the unfused ops).  The op codes are packed in
// `code` (kernel arguments in few SGPRs): mode l at bits 2l, bin i at 8 + 3i, sf i at 17 + 4i,
// swap at 29.
struct ExprArgs {
  const float* p[4];
  int ld[4];
  int code;
};

__host__ __device__ constexpr int ex_mode(int code, int l) { return (code >> (2 * l)) & 3; }
__host__ __device__ constexpr int ex_bin(int code, int i) { return (code >> (8 + 3 * i)) & 7; }
__host__ __device__ constexpr int ex_sf(int code, int i) { return (code >> (17 + 4 * i)) & 15; }
__host__ __device__ constexpr int ex_swap(int code) { return (code >> 29) & 1; }

template <int XMODE>
constexpr int expr_leaves() { return XMODE == XM_EX1 ? 2 : (XMODE == XM_EX2 ? 3 : (XMODE == XM_EX3 ? 4 : 0)); }

// d[k] = a[k] bin b[k] over M values (bin NONE: d = a), bin_apply's arithmetic
template <int M>
__device__ __forceinline__ void bin_arr(int bin, float* d, const float* a, const float* b) {
#pragma clang fp contract(off)
  switch (bin) {
    case GTA_BIN_ADD:
#pragma unroll
      for (int k = 0; k < M; ++k) d[k] = bin_apply(GTA_BIN_ADD, a[k], b[k]);
      break;
    case GTA_BIN_MUL:
#pragma unroll
      for (int k = 0; k < M; ++k) d[k] = bin_apply(GTA_BIN_MUL, a[k], b[k]);
      break;
    case GTA_BIN_DIV:
#pragma unroll
      for (int k = 0; k < M; ++k) d[k] = bin_apply(GTA_BIN_DIV, a[k], b[k]);
      break;
    case GTA_BIN_SUB:
#pragma unroll
      for (int k = 0; k < M; ++k) d[k] = bin_apply(GTA_BIN_SUB, a[k], b[k]);
      break;
    default:
#pragma unroll
      for (int k = 0; k < M; ++k) d[k] = a[k];
  }
}

// d[k] = sf(d[k]) over M values, sf_apply's arithmetic
template <int M>
__device__ __forceinline__ void sf_arr(int sf, float* d) {
#pragma clang fp contract(off)
#define GTA_SF_CASE(K_)                                              \
  case K_:                                                           \
    _Pragma("unroll") for (int k = 0; k < M; ++k) d[k] = sf_apply(K_, d[k]); \
    break;
  switch (sf) {
    GTA_SF_CASE(GTA_SF_RELU) GTA_SF_CASE(GTA_SF_EXP_LEAKY_RELU) GTA_SF_CASE(GTA_SF_ELU) GTA_SF_CASE(GTA_SF_EXP)
    GTA_SF_CASE(GTA_SF_LEAKY_RELU) GTA_SF_CASE(GTA_SF_SIGMOID) GTA_SF_CASE(GTA_SF_TANH) GTA_SF_CASE(GTA_SF_RECIP)
    default: break;  // GTA_SF_NONE
  }
#undef GTA_SF_CASE
}

// the expression over one unrolled step: L[l] = operand l's M values, t = the edge values
template <int XMODE, int M>
__device__ __forceinline__ void expr_eval(int code, float (&L)[4][M], float* t) {
  float u[M];
  bin_arr<M>(ex_bin(code, 0), u, L[0], L[1]);
  sf_arr<M>(ex_sf(code, 0), u);
  if constexpr (XMODE == XM_EX1) {
#pragma unroll
    for (int k = 0; k < M; ++k) t[k] = u[k];
  } else if constexpr (XMODE == XM_EX2) {
    if (ex_swap(code)) bin_arr<M>(ex_bin(code, 1), t, L[2], u);
    else bin_arr<M>(ex_bin(code, 1), t, u, L[2]);
    sf_arr<M>(ex_sf(code, 1), t);
  } else {
    float v[M];
    bin_arr<M>(ex_bin(code, 1), v, L[2], L[3]);
    sf_arr<M>(ex_sf(code, 1), v);
    bin_arr<M>(ex_bin(code, 2), t, u, v);
    sf_arr<M>(ex_sf(code, 2), t);
  }
}

// WM_EDGE1: one weight per edge (H = 1: GCN's 1/sqrt(d_i d_j), GIN's edge operand) -- 64 weights
// per coalesced load beside the 64 indices, broadcast to the edge's lanes like its index, instead of
// one weight load per lane and edge (WM_HEAD's path, which doubles the vector-memory instructions
// of a narrow row); the same product and sum per element, so bitwise equal to WM_HEAD at H = 1
enum { WM_NONE = 0, WM_HEAD = 1, WM_FULL = 2, WM_EDGE1 = 3 };

// Shared parts of the per-row gather kernels (k_aggregate, k_reduce, k_agg_lean, k_agg_expr).
// A wave's work item: a whole row, or with a plan a <= chunk slice [eb, ee) of one; split: the
// row has several items, each writing a partial that a combine kernel folds.
struct WorkItem {
  int64_t row, eb, ee;
  bool split;
};

__device__ __forceinline__ WorkItem work_item(const int64_t* __restrict__ indptr, const PlanView& plan, int use_plan,
                                              int64_t item) {
  if (use_plan) {
    const int32_t ir = plan.item_row[item];
    return {ir & 0x7fffffff, plan.item_beg[item], plan.item_end[item], ir < 0};
  }
  return {item, indptr[item], indptr[item + 1], false};
}

// one piece of the generic form: VW elements of the row from column c on (valid: inside the row)
struct Piece {
  int col, lo;
  bool valid;
};

template <int VW>
__device__ __forceinline__ Piece piece_at(int c, int F) {
  Piece p{c < F ? c : 0, 0, c < F};
  if constexpr (VW == 8) {  // 16-B bf16 pieces, F % 4 == 0: the last lane's piece starts 4 early
    if (p.valid && p.col + VW > F) { p.lo = p.col + VW - F; p.col -= p.lo; }  // (its first lo values unused)
  }
  return p;
}

// the row that edge e0 + jj of the item gathers; idxv: this block's 64 source indices, one per lane
template <int LPE, int XMODE>
__device__ __forceinline__ int64_t gather_row(int64_t e0, int jj, int64_t row, int x_is_row, int idxv) {
  if (XMODE == XM_EDGE) return e0 + jj;
  if (x_is_row) return row;
  if (LPE == kWave) return __builtin_amdgcn_readlane(idxv, jj);
  return __shfl(idxv, jj);
}

// a piece whose first lo values belong to the lane before: store its upper half only
template <int VW>
__device__ __forceinline__ void store_piece(const Vec<VW>& o, float* p, int lo) {
  if constexpr (VW == 8) {
    if (lo) { *reinterpret_cast<float4*>(p + 4) = make_float4(o.v[4], o.v[5], o.v[6], o.v[7]); return; }
  }
  o.store(p);
}

// TX: the gathered rows' element type (float, or bf16 as uint16_t: widened exactly, fp32 sums)
template <int LPE, int VW, int NV, int XMODE, int WMODE, typename TX = float, int URX = 0>
__global__ void __launch_bounds__(kBlock)
k_aggregate(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
            PlanView plan, int use_plan, int64_t chunk, int x_is_row,
            const TX* __restrict__ x, int64_t ldx, int F,
            const float* __restrict__ w, int64_t ldw, int gsz,
            const float* __restrict__ row_scale, float* __restrict__ y, int64_t ldy, int accumulate,
            float* __restrict__ partial, const TX* __restrict__ xs = nullptr, int64_t ldxs = 0,
            const float* __restrict__ self_scale = nullptr, int y_bf16 = 0, const ExprArgs ex = ExprArgs{}) {
  // xs (gta_aggregate_self): y[row] = self_scale * xs[row] + row_scale[row] * sum, the self term
  // formed exactly as an applynode MUL by a broadcast scalar would (GIN op 3 + op 4).
  // y_bf16: y holds bf16 (RNE of the fp32 value; ldy in bf16 elements) -- for a consumer that rounds
  // its input to bf16 anyway (the fused GIN MLP), so the rounding happens once, here
  // ex (XMODE XM_EX*): the edge value is an apply_edge expression of ex's operands (see ExprArgs)
  constexpr int EPI = kWave / LPE;                 // edges per wave instruction
  constexpr int NL = expr_leaves<XMODE>();         // expression operands (0: a plain gather)
  // row loads in flight per lane: ~64 B of each lane's rows per unrolled step (an expression
  // gathers up to NL rows per edge: ~32 B of each)
  constexpr int XB = NV * VW * static_cast<int>(sizeof(TX));
  constexpr int RB = NL ? 32 : 64;
  constexpr int UR = URX ? URX : ((RB / XB) < 2 ? 2 : ((RB / XB) > 8 ? 8 : RB / XB));
  constexpr int STEP = UR * EPI;                    // edges per unrolled step
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  const int64_t n_items = use_plan ? plan.hdr[0] : n_rows;
  if (item >= n_items) return;

  const auto [row, eb, ee, split] = work_item(indptr, plan, use_plan, item);
  const int sub = (LPE == kWave) ? 0 : lane / LPE;
  const int cl = (LPE == kWave) ? lane : lane % LPE;
  const float scale = (row_scale != nullptr && !split) ? row_scale[row] : 1.f;

  for (int c0 = 0; c0 < F; c0 += LPE * VW * NV) {
    int col[NV], hcol[NV], lo[NV];
    bool cval[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const Piece p = piece_at<VW>(c0 + (v * LPE + cl) * VW, F);
      col[v] = p.col; lo[v] = p.lo; cval[v] = p.valid;
      hcol[v] = (WMODE == WM_HEAD) ? col[v] / gsz : 0;
    }
    float acc[NV][VW];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int k = 0; k < VW; ++k) acc[v][k] = 0.f;

    // source indices arrive 64 at a time; the next block's are prefetched while
    // this block's rows are in flight (clamped address: the load is unconditional)
    const bool use_idx = ((XMODE == XM_IDX) && !x_is_row) || NL > 0;
    int idxv = 0;
    float wv = 0.f;
    if (use_idx && eb < ee) idxv = indices[min(eb + lane, ee - 1)];
    if (WMODE == WM_EDGE1 && eb < ee) wv = w[min(eb + lane, ee - 1) * ldw];
    for (int64_t e0 = eb; e0 < ee; e0 += kWave) {
      const int n = static_cast<int>(min<int64_t>(kWave, ee - e0));
      int idxn = 0;
      float wn = 0.f;
      if (use_idx) idxn = indices[min(e0 + kWave + lane, ee - 1)];
      if (WMODE == WM_EDGE1) wn = w[min(e0 + kWave + lane, ee - 1) * ldw];
      for (int s = 0; s < n; s += STEP) {
        Vec<VW> xv[UR][NV];
        float wh[UR][NV];
        Vec<VW> wf[(WMODE == WM_FULL) ? UR : 1][(WMODE == WM_FULL) ? NV : 1];
        float lv[4][NL ? UR * NV * VW : 1];  // an expression's operand values per edge
        bool valid[UR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
          const int j = s + u * EPI + sub;
          valid[u] = j < n;
          const int jj = j < n ? j : n - 1;
          if constexpr (NL > 0) {
            const int64_t sr = (LPE == kWave) ? __builtin_amdgcn_readlane(idxv, jj) : __shfl(idxv, jj);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
              // straight-line: every operand loaded per edge at a uniform address (a DST row or a
              // broadcast row repeats within the item: L1 hits), no branch between the loads
              const int md = ex_mode(ex.code, l);
              const int64_t r = md == GTA_IDX_SRC ? sr : (md == GTA_IDX_DST ? row : e0 + jj);
              const float* p = ex.p[l] + r * static_cast<int64_t>(ex.ld[l]);
              Vec<VW> q[NV];
#pragma unroll
              for (int v = 0; v < NV; ++v) q[v].load(p + col[v]);
#pragma unroll
              for (int v = 0; v < NV; ++v)
#pragma unroll
                for (int k = 0; k < VW; ++k) lv[l][(u * NV + v) * VW + k] = q[v].v[k];
            }
            continue;
          }
          const TX* xp = x + gather_row<LPE, XMODE>(e0, jj, row, x_is_row, idxv) * ldx;
#pragma unroll
          for (int v = 0; v < NV; ++v) load_row(xv[u][v], xp + col[v]);
          if (WMODE == WM_HEAD) {
            const float* wp = w + (e0 + jj) * ldw;
#pragma unroll
            for (int v = 0; v < NV; ++v) wh[u][v] = wp[hcol[v]];
          } else if (WMODE == WM_EDGE1) {
            const float we = (LPE == kWave)
                                 ? __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wv), jj))
                                 : __shfl(wv, jj);
#pragma unroll
            for (int v = 0; v < NV; ++v) wh[u][v] = we;
          } else if (WMODE == WM_FULL) {
            const float* wp = w + (e0 + jj) * ldw;
#pragma unroll
            for (int v = 0; v < NV; ++v) wf[u][v].load(wp + col[v]);
          }
        }
        if constexpr (NL > 0) {
          float t[UR * NV * VW];
          expr_eval<XMODE, UR * NV * VW>(ex.code, lv, t);
#pragma unroll
          for (int u = 0; u < UR; ++u)
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
              for (int k = 0; k < VW; ++k) xv[u][v].v[k] = t[(u * NV + v) * VW + k];
        }
#pragma unroll
        for (int u = 0; u < UR; ++u) {
#pragma unroll
          for (int v = 0; v < NV; ++v) {
#pragma unroll
            for (int k = 0; k < VW; ++k) {
              float t;
              if (WMODE == WM_HEAD || WMODE == WM_EDGE1) t = wh[u][v] * xv[u][v].v[k];
              else if (WMODE == WM_FULL) t = wf[u][v].v[k] * xv[u][v].v[k];
              else t = xv[u][v].v[k];
              acc[v][k] += valid[u] ? t : 0.f;
            }
          }
        }
      }
      idxv = idxn;
      wv = wn;
    }
    if (LPE < kWave) {  // fold the EPI edge slots (fixed butterfly order)
#pragma unroll
      for (int off = LPE; off < kWave; off <<= 1)
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int k = 0; k < VW; ++k) acc[v][k] += __shfl_xor(acc[v][k], off);
    }
    if (sub == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (!cval[v]) continue;
        Vec<VW> o;
        // store_piece's rule, written out as a lambda: with the helper inlined here the compiler
        // packs the edge loop's adds and multiplies differently (the 16-B form's came out scalar)
        auto put = [&](float* p) {
          if constexpr (VW == 8) {
            if (lo[v]) { *reinterpret_cast<float4*>(p + 4) = make_float4(o.v[4], o.v[5], o.v[6], o.v[7]); return; }
          }
          o.store(p);
        };
        if (split) {
#pragma unroll
          for (int k = 0; k < VW; ++k) o.v[k] = acc[v][k];
          put(partial + item * static_cast<int64_t>(F) + col[v]);
        } else {
          float* yp = y + row * ldy + col[v];
          if (accumulate) {
            Vec<VW> old;
            old.load(yp);
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = old.v[k] + scale * acc[v][k];
          } else if (xs != nullptr) {
#pragma clang fp contract(off)
            // no fma contraction: each product rounded, as the unfused MUL and aggregate store them
            Vec<VW> sv;
            load_row(sv, xs + row * ldxs + col[v]);
            const float ss = self_scale ? *self_scale : 1.f;
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = sv.v[k] * ss + scale * acc[v][k];
          } else {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = scale * acc[v][k];
          }
          if (y_bf16) {
            uint16_t* yb = reinterpret_cast<uint16_t*>(y) + row * ldy + col[v];
#pragma unroll
            for (int k = 0; k < VW; ++k)
              if (k >= lo[v]) yb[k] = to_bf16_bits(o.v[k]);
          } else {
            put(yp);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K2' reduce: the gather whose COMP_TYPE is MAX or MIN (gta_reduce).
//   k_aggregate's generic form (its work_item, piece_at, gather_row and store_piece) with the
//   reducer in place of the fma: idle edge slots and the < STEP remainder hold the identity (-inf),
//   the LPE < 64 butterfly folds with the reducer, split rows write their partial maxima and
//   k_reduce_combine folds them (any order gives the same value).
//   MIN runs as -max(-x): sbit (0 or the sign bit, wave-uniform) flips every value on its way in
//   and the result on its way out, which is exact, so one instantiation serves both.
//   red_max propagates NaN (an explicit compare-and-select plus the unordered test; fmaxf would
//   drop it, and with it the guard-band arena's poison) and picks one of its operands' bits.
//   A row without edges gets 0, decided by its degree.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float red_max(float a, float t) { return (t > a || t != t) ? t : a; }
__device__ __forceinline__ float red_flip(float v, uint32_t sbit) { return __uint_as_float(__float_as_uint(v) ^ sbit); }

template <int LPE, int VW, int NV, int XMODE, typename TX = float>
__global__ void __launch_bounds__(kBlock)
k_reduce(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, PlanView plan,
         int use_plan, int x_is_row, const TX* __restrict__ x, int64_t ldx, int F, uint32_t sbit,
         float* __restrict__ y, int64_t ldy, float* __restrict__ partial) {
  constexpr int EPI = kWave / LPE;  // edges per wave instruction
  constexpr int XB = NV * VW * static_cast<int>(sizeof(TX));
  constexpr int UR = (64 / XB) < 2 ? 2 : ((64 / XB) > 8 ? 8 : 64 / XB);  // ~64 B of rows in flight per lane
  constexpr int STEP = UR * EPI;
  const float ident = -__builtin_inff();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  const int64_t n_items = use_plan ? plan.hdr[0] : n_rows;
  if (item >= n_items) return;

  const auto [row, eb, ee, split] = work_item(indptr, plan, use_plan, item);
  const bool empty = eb >= ee;  // a whole row without edges (an item of a split row is never empty)
  const int sub = (LPE == kWave) ? 0 : lane / LPE;
  const int cl = (LPE == kWave) ? lane : lane % LPE;

  for (int c0 = 0; c0 < F; c0 += LPE * VW * NV) {
    int col[NV], lo[NV];
    bool cval[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const Piece p = piece_at<VW>(c0 + (v * LPE + cl) * VW, F);
      col[v] = p.col; lo[v] = p.lo; cval[v] = p.valid;
    }
    float acc[NV][VW];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int k = 0; k < VW; ++k) acc[v][k] = ident;

    const bool use_idx = (XMODE == XM_IDX) && !x_is_row;
    int idxv = 0;
    if (use_idx && eb < ee) idxv = indices[min(eb + lane, ee - 1)];
    for (int64_t e0 = eb; e0 < ee; e0 += kWave) {
      const int n = static_cast<int>(min<int64_t>(kWave, ee - e0));
      int idxn = 0;
      if (use_idx) idxn = indices[min(e0 + kWave + lane, ee - 1)];  // clamped: the load is unconditional
      for (int s = 0; s < n; s += STEP) {
        Vec<VW> xv[UR][NV];
        bool valid[UR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
          const int j = s + u * EPI + sub;
          valid[u] = j < n;
          const int jj = j < n ? j : n - 1;
          const TX* xp = x + gather_row<LPE, XMODE>(e0, jj, row, x_is_row, idxv) * ldx;
#pragma unroll
          for (int v = 0; v < NV; ++v) load_row(xv[u][v], xp + col[v]);
        }
#pragma unroll
        for (int u = 0; u < UR; ++u)
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < VW; ++k)
              acc[v][k] = red_max(acc[v][k], valid[u] ? red_flip(xv[u][v].v[k], sbit) : ident);
      }
      idxv = idxn;
    }
    if (LPE < kWave) {  // fold the EPI edge slots with the reducer
#pragma unroll
      for (int off = LPE; off < kWave; off <<= 1)
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int k = 0; k < VW; ++k) acc[v][k] = red_max(acc[v][k], __shfl_xor(acc[v][k], off));
    }
    if (sub == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (!cval[v]) continue;
        Vec<VW> o;
        // a split item's partial stays in the max domain (k_reduce_combine flips the folded value)
#pragma unroll
        for (int k = 0; k < VW; ++k) o.v[k] = split ? acc[v][k] : (empty ? 0.f : red_flip(acc[v][k], sbit));
        store_piece(o, split ? partial + item * static_cast<int64_t>(F) + col[v] : y + row * ldy + col[v], lo[v]);
      }
    }
  }
}

// fold the chunk partials of split rows (max domain) and flip the result back
__global__ void __launch_bounds__(kBlock)
k_reduce_combine(PlanView plan, int F, uint32_t sbit, float* __restrict__ y, int64_t ldy,
                 const float* __restrict__ partial) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (s >= plan.hdr[1]) return;
  const int64_t row = plan.split_row[s];
  const int64_t first = plan.split_first[s];
  const int cnt = plan.split_cnt[s];
  for (int c = lane; c < F; c += kWave) {
    float a = -__builtin_inff();
    for (int j = 0; j < cnt; ++j) a = red_max(a, partial[(first + j) * F + c]);
    y[row * ldy + c] = red_flip(a, sbit);
  }
}

// ---------------------------------------------------------------------------
// K2'' multi-reducer: one pass over a row's edges fills MEAN / MAX / MIN / VAR / STD
// (gta_reduce_multi, PNA's aggregators over the same messages).
//   k_reduce's skeleton with up to four accumulator sets per column, specialised at compile time
//   on MOM (the moments s1, s2) and EXT (the extrema), so no instantiation carries dead ones; which
//   outputs are stored is a wave-uniform run-time choice (a NULL pointer in MultiOut).
//   Moments: about the shift k(i, c) = the operand value at the row's FIRST edge (CSR position
//   indptr[i]): s1 = sum (x - k), s2 = sum (x - k)^2 in fp32, then MEAN = k + s1/d,
//   VAR = max(s2/d - (s1/d)^2, 0), STD = sqrt(VAR + eps).  The terms are the spread's size, not the
//   mean's, so the subtraction in VAR cancels nothing that matters (the unshifted E[x^2] - E[x]^2
//   loses every digit once |mean| >> std).  An item of a split row reads the row's first edge
//   itself, so all of a row's items use one k and their partial sums add up.
//   Extrema: red_max as in k_reduce; MIN is carried as max(-x) in its own accumulator, the same
//   compare on the same values, so both are bitwise gta_reduce's.
//   A sum s2 that is not finite (a +-inf operand, or squares past fp32) makes the three moment
//   outputs NaN.  A row without edges gets 0 in every output, decided by its degree.
//   Split rows store P = 2 MOM + 2 EXT planes of partials ([items, F] each, pstride apart):
//   s1, s2, then max, max(-x); k_reduce_multi_combine sums / folds them in item order.
// ---------------------------------------------------------------------------
enum { MR_MEAN = 0, MR_MAX = 1, MR_MIN = 2, MR_VAR = 3, MR_STD = 4, MR_N = 5 };
struct MultiOut {  // the outputs in GTA_MR_* bit order; y NULL: not requested
  float* y[MR_N];
  int64_t ld[MR_N];
};

struct Moments {
  float mean, var, sd;
};
__device__ __forceinline__ Moments moments_of(float k, float s1, float s2, float deg, float eps) {
  const float bad = s2 - s2;  // 0, or NaN once s2 is not finite
  const float m = s1 / deg;
  float var = s2 / deg - m * m;
  var = (var < 0.f ? 0.f : var) + bad;  // the select keeps a NaN
  return {k + m + bad, var, sqrtf(var + eps)};
}

// the row of x that holds row's shift: the operand of its first edge (CSR position first)
template <int XMODE>
__device__ __forceinline__ int64_t shift_row(const int32_t* __restrict__ indices, int64_t first, int64_t row,
                                             int x_is_row) {
  if (XMODE == XM_EDGE) return first;
  return x_is_row ? row : static_cast<int64_t>(indices[first]);
}

template <int LPE, int VW, int NV, int XMODE, bool MOM, bool EXT, typename TX = float>
__global__ void __launch_bounds__(kBlock)
k_reduce_multi(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, PlanView plan,
               int use_plan, int x_is_row, const TX* __restrict__ x, int64_t ldx, int F, MultiOut out, float eps,
               float* __restrict__ partial, int64_t pstride) {
  constexpr int EPI = kWave / LPE;  // edges per wave instruction
  constexpr int XB = NV * VW * static_cast<int>(sizeof(TX));
  constexpr int UR = (64 / XB) < 2 ? 2 : ((64 / XB) > 8 ? 8 : 64 / XB);  // ~64 B of rows in flight per lane
  constexpr int STEP = UR * EPI;
  constexpr uint32_t kSign = 0x80000000u;
  const float ident = -__builtin_inff();
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  const int64_t n_items = use_plan ? plan.hdr[0] : n_rows;
  if (item >= n_items) return;

  const auto [row, eb, ee, split] = work_item(indptr, plan, use_plan, item);
  const bool empty = eb >= ee;  // a whole row without edges (an item of a split row is never empty)
  const int sub = (LPE == kWave) ? 0 : lane / LPE;
  const int cl = (LPE == kWave) ? lane : lane % LPE;
  const float deg = static_cast<float>(ee - eb);  // a row in one item: its degree

  for (int c0 = 0; c0 < F; c0 += LPE * VW * NV) {
    int col[NV], lo[NV];
    bool cval[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const Piece p = piece_at<VW>(c0 + (v * LPE + cl) * VW, F);
      col[v] = p.col; lo[v] = p.lo; cval[v] = p.valid;
    }
    float s1[NV][VW], s2[NV][VW], amx[NV][VW], amn[NV][VW];
    Vec<VW> kv[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        s1[v][k] = 0.f; s2[v][k] = 0.f; kv[v].v[k] = 0.f;
        amx[v][k] = ident; amn[v][k] = ident;
      }
    if (MOM && !empty) {
      const TX* kp = x + shift_row<XMODE>(indices, split ? indptr[row] : eb, row, x_is_row) * ldx;
#pragma unroll
      for (int v = 0; v < NV; ++v) load_row(kv[v], kp + col[v]);
    }

    const bool use_idx = (XMODE == XM_IDX) && !x_is_row;
    int idxv = 0;
    if (use_idx && eb < ee) idxv = indices[min(eb + lane, ee - 1)];
    for (int64_t e0 = eb; e0 < ee; e0 += kWave) {
      const int n = static_cast<int>(min<int64_t>(kWave, ee - e0));
      int idxn = 0;
      if (use_idx) idxn = indices[min(e0 + kWave + lane, ee - 1)];  // clamped: the load is unconditional
      for (int s = 0; s < n; s += STEP) {
        Vec<VW> xv[UR][NV];
        bool valid[UR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
          const int j = s + u * EPI + sub;
          valid[u] = j < n;
          const int jj = j < n ? j : n - 1;
          const TX* xp = x + gather_row<LPE, XMODE>(e0, jj, row, x_is_row, idxv) * ldx;
#pragma unroll
          for (int v = 0; v < NV; ++v) load_row(xv[u][v], xp + col[v]);
        }
#pragma unroll
        for (int u = 0; u < UR; ++u)
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < VW; ++k) {
              const float t = xv[u][v].v[k];
              if constexpr (MOM) {
                const float d = valid[u] ? t - kv[v].v[k] : 0.f;
                s1[v][k] += d;
                s2[v][k] = fmaf(d, d, s2[v][k]);
              }
              if constexpr (EXT) {
                amx[v][k] = red_max(amx[v][k], valid[u] ? t : ident);
                amn[v][k] = red_max(amn[v][k], valid[u] ? red_flip(t, kSign) : ident);
              }
            }
      }
      idxv = idxn;
    }
    if (LPE < kWave) {  // fold the EPI edge slots: the sums add, the extrema fold with the reducer
#pragma unroll
      for (int off = LPE; off < kWave; off <<= 1)
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
          for (int k = 0; k < VW; ++k) {
            if constexpr (MOM) {
              s1[v][k] += __shfl_xor(s1[v][k], off);
              s2[v][k] += __shfl_xor(s2[v][k], off);
            }
            if constexpr (EXT) {
              amx[v][k] = red_max(amx[v][k], __shfl_xor(amx[v][k], off));
              amn[v][k] = red_max(amn[v][k], __shfl_xor(amn[v][k], off));
            }
          }
    }
    if (sub == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        if (!cval[v]) continue;
        Vec<VW> o;
        if (split) {  // the planes of partials: sums as they are, both extrema in the max domain
          float* pp = partial + item * static_cast<int64_t>(F) + col[v];
          if constexpr (MOM) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = s1[v][k];
            store_piece(o, pp, lo[v]);
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = s2[v][k];
            store_piece(o, pp + pstride, lo[v]);
            pp += 2 * pstride;
          }
          if constexpr (EXT) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = amx[v][k];
            store_piece(o, pp, lo[v]);
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = amn[v][k];
            store_piece(o, pp + pstride, lo[v]);
          }
          continue;
        }
        if constexpr (MOM) {
          Moments m[VW];
#pragma unroll
          for (int k = 0; k < VW; ++k) m[k] = moments_of(kv[v].v[k], s1[v][k], s2[v][k], deg, eps);
          if (out.y[MR_MEAN]) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = empty ? 0.f : m[k].mean;
            store_piece(o, out.y[MR_MEAN] + row * out.ld[MR_MEAN] + col[v], lo[v]);
          }
          if (out.y[MR_VAR]) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = empty ? 0.f : m[k].var;
            store_piece(o, out.y[MR_VAR] + row * out.ld[MR_VAR] + col[v], lo[v]);
          }
          if (out.y[MR_STD]) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = empty ? 0.f : m[k].sd;
            store_piece(o, out.y[MR_STD] + row * out.ld[MR_STD] + col[v], lo[v]);
          }
        }
        if constexpr (EXT) {
          if (out.y[MR_MAX]) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = empty ? 0.f : amx[v][k];
            store_piece(o, out.y[MR_MAX] + row * out.ld[MR_MAX] + col[v], lo[v]);
          }
          if (out.y[MR_MIN]) {
#pragma unroll
            for (int k = 0; k < VW; ++k) o.v[k] = empty ? 0.f : red_flip(amn[v][k], kSign);
            store_piece(o, out.y[MR_MIN] + row * out.ld[MR_MIN] + col[v], lo[v]);
          }
        }
      }
    }
  }
}

// split rows: sum the two planes of moment partials in item order and fold the two planes of
// extrema (k_reduce_combine's fold), then the same epilogue; the row's shift is read again
template <bool MOM, bool EXT, typename TX>
__global__ void __launch_bounds__(kBlock)
k_reduce_multi_combine(PlanView plan, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                       int x_mode, const TX* __restrict__ x, int64_t ldx, int F, MultiOut out, float eps,
                       const float* __restrict__ partial, int64_t pstride) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (s >= plan.hdr[1]) return;
  const int64_t row = plan.split_row[s];
  const int64_t first = plan.split_first[s];
  const int cnt = plan.split_cnt[s];
  const int64_t e = indptr[row];
  const float deg = static_cast<float>(indptr[row + 1] - e);  // a split row has edges
  const TX* kp = x;
  if (MOM) kp += (x_mode == GTA_IDX_EDGE ? e : (x_mode == GTA_IDX_DST ? row : static_cast<int64_t>(indices[e]))) * ldx;
  for (int c = lane; c < F; c += kWave) {
    const float* pp = partial + first * F + c;
    if constexpr (MOM) {
      float s1 = 0.f, s2 = 0.f;
      for (int j = 0; j < cnt; ++j) {
        s1 += pp[static_cast<int64_t>(j) * F];
        s2 += pp[pstride + static_cast<int64_t>(j) * F];
      }
      const Moments m = moments_of(load_elem(kp + c), s1, s2, deg, eps);
      if (out.y[MR_MEAN]) out.y[MR_MEAN][row * out.ld[MR_MEAN] + c] = m.mean;
      if (out.y[MR_VAR]) out.y[MR_VAR][row * out.ld[MR_VAR] + c] = m.var;
      if (out.y[MR_STD]) out.y[MR_STD][row * out.ld[MR_STD] + c] = m.sd;
      pp += 2 * pstride;
    }
    if constexpr (EXT) {
      float amx = -__builtin_inff(), amn = -__builtin_inff();
      for (int j = 0; j < cnt; ++j) {
        amx = red_max(amx, pp[static_cast<int64_t>(j) * F]);
        amn = red_max(amn, pp[pstride + static_cast<int64_t>(j) * F]);
      }
      if (out.y[MR_MAX]) out.y[MR_MAX][row * out.ld[MR_MAX] + c] = amx;
      if (out.y[MR_MIN]) out.y[MR_MIN][row * out.ld[MR_MIN] + c] = red_flip(amn, 0x80000000u);
    }
  }
}

// ---------------------------------------------------------------------------
// Lean aggregate for rows that exactly fill a wavefront (F = 64 * VW): one edge
// per wave instruction, wave-uniform row base.  Per unrolled step of U edges:
//   * U row loads issued back to back, no per-edge validity select (full steps
//     only; the < U remainder runs a separate one-edge loop);
//   * weights (heads mode, GL = lanes per head = (F/H)/VW) come in ONE coalesced
//     load per GL edges in a head-transposed layout -- lane l holds
//     w[e0 + (l % GL), l / GL], i.e. its own head for GL different edges -- and
//     each edge's weight reaches its head's lanes by a ds_swizzle broadcast
//     inside the GL-lane group (no memory traffic, no VMEM per edge);
//   * fma accumulation in edge order (deterministic).
// GL = 0: unweighted.
// ---------------------------------------------------------------------------
template <int G, int K>
__device__ __forceinline__ float group_bcast(float v) {  // lane (l & ~(G-1)) | K of each G-lane group
  constexpr int pattern = (0x1F & ~(G - 1)) | ((K % G) << 5);
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), pattern));
}

template <int G, int U>
__device__ __forceinline__ void bcast_all(const float* wa, float* out) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float v = wa[u / G];
    switch (u % G) {  // ds_swizzle needs a literal pattern
#define GTA_BC(k) case k: out[u] = group_bcast<G, k>(v); break;
      GTA_BC(0) GTA_BC(1) GTA_BC(2) GTA_BC(3) GTA_BC(4) GTA_BC(5) GTA_BC(6) GTA_BC(7)
      GTA_BC(8) GTA_BC(9) GTA_BC(10) GTA_BC(11) GTA_BC(12) GTA_BC(13) GTA_BC(14) GTA_BC(15)
#undef GTA_BC
    }
  }
}

// acc[VW] = the lean sum over edges [eb, ee) of lane's VW columns (k_agg_lean, k_agg_seg2d)
template <int VW, int GL>
__device__ __forceinline__ void lean_gather_sum(const int32_t* __restrict__ indices, int64_t eb, int64_t ee,
                                                const float* __restrict__ x, int64_t ldx,
                                                const float* __restrict__ w, int64_t ldw, int lane, float (&acc)[VW]) {
  constexpr int U = (GL > 8) ? GL : 8;               // edges per unrolled step
  constexpr int NWL = (GL > 0) ? U / GL : 0;         // weight loads per step
  const int col = lane * VW;
  const int head = (GL > 0) ? lane / GL : 0;      // this lane's head (F/H = GL * VW columns)
  const int gsub = (GL > 0) ? lane % GL : 0;      // which edge of a GL-block this lane loads the weight of
#pragma unroll
  for (int k = 0; k < VW; ++k) acc[k] = 0.f;

  int idxv = (eb < ee) ? indices[min(eb + lane, ee - 1)] : 0;
  for (int64_t e0 = eb; e0 < ee; e0 += kWave) {
    const int n = static_cast<int>(min<int64_t>(kWave, ee - e0));
    const int idxn = indices[min(e0 + kWave + lane, ee - 1)];  // prefetch next block (clamped)
    const float* wblk = (GL > 0) ? w + e0 * ldw : nullptr;
    int s = 0;
    for (; s + U <= n; s += U) {
      Vec<VW> xv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t xr = __builtin_amdgcn_readlane(idxv, s + u);
        xv[u].load(x + xr * ldx + col);
      }
      if (GL > 0) {
        float wa[NWL > 0 ? NWL : 1], wu[U];
#pragma unroll
        for (int q = 0; q < NWL; ++q) wa[q] = wblk[static_cast<int64_t>(s + q * GL + gsub) * ldw + head];
        bcast_all<(GL > 0 ? GL : 1), U>(wa, wu);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < VW; ++k) acc[k] = fmaf(wu[u], xv[u].v[k], acc[k]);
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < VW; ++k) acc[k] += xv[u].v[k];
      }
    }
    for (; s < n; ++s) {  // remainder, one edge at a time
      const int64_t xr = __builtin_amdgcn_readlane(idxv, s);
      Vec<VW> xv;
      xv.load(x + xr * ldx + col);
      const float wv = (GL > 0) ? wblk[static_cast<int64_t>(s) * ldw + head] : 1.f;
#pragma unroll
      for (int k = 0; k < VW; ++k) acc[k] = (GL > 0) ? fmaf(wv, xv.v[k], acc[k]) : acc[k] + xv.v[k];
    }
    idxv = idxn;
  }
}

struct SegItem {  // one (column block, row) work item of the blocked plan: 16 B, loaded with one dwordx4
  int64_t beg;
  int32_t row;
  int32_t len;
};

template <int VW, int GL>
__global__ void __launch_bounds__(kBlock)
k_agg_lean(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, PlanView plan,
           int use_plan, int64_t chunk, const float* __restrict__ x, int64_t ldx, int F,
           const float* __restrict__ w, int64_t ldw, const float* __restrict__ row_scale,
           float* __restrict__ y, int64_t ldy, int accumulate, float* __restrict__ partial,
           const float* __restrict__ xs = nullptr, int64_t ldxs = 0, const float* __restrict__ self_scale = nullptr) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  const int64_t n_items = use_plan ? plan.hdr[0] : n_rows;
  if (item >= n_items) return;
  const auto [row, eb, ee, split] = work_item(indptr, plan, use_plan, item);
  const int col = lane * VW;
  float acc[VW];
  lean_gather_sum<VW, GL>(indices, eb, ee, x, ldx, w, ldw, lane, acc);
  Vec<VW> o;
  if (split) {
#pragma unroll
    for (int k = 0; k < VW; ++k) o.v[k] = acc[k];
    o.store(partial + item * static_cast<int64_t>(F) + col);
  } else {
    const float scale = row_scale ? row_scale[row] : 1.f;
    float* yp = y + row * ldy + col;
    if (accumulate) {
      Vec<VW> old;
      old.load(yp);
#pragma unroll
      for (int k = 0; k < VW; ++k) o.v[k] = old.v[k] + scale * acc[k];
    } else if (xs != nullptr) {  // gta_aggregate_self's term, as k_aggregate forms it (written out in
      // both kernels: behind a shared helper the compiler contracts `old + scale * acc` differently)
#pragma clang fp contract(off)
      Vec<VW> sv;
      sv.load(xs + row * ldxs + col);
      const float ss = self_scale ? *self_scale : 1.f;
#pragma unroll
      for (int k = 0; k < VW; ++k) o.v[k] = sv.v[k] * ss + scale * acc[k];
    } else {
#pragma unroll
      for (int k = 0; k < VW; ++k) o.v[k] = scale * acc[k];
    }
    o.store(yp);
  }
}

// gta_aggregate_expr for rows that exactly fill a wavefront (F = 128 at 8 B per lane, F = 256 at
// 16 B: the shapes where k_aggregate's XM_EDGE form, the unfused gather, runs one edge per wave
// instruction): U edges per step with every operand load of the step issued back to back at
// addresses hoisted per item (a per-operand base and the index that scales its stride), one
// expression pass over the step, then the same masked in-order sum as k_aggregate -- bitwise its
// result.  The generic k_aggregate XM_EX* form spent ~20 scalar instructions selecting each load's
// row and took 3 steps for a 10-edge row.
// CM >= 0: the row-constant operands as a compile-time mask (bit l: operand l), so those operands
// take no registers beside their one copy and no branch in the step; CM = -1: read from ex.
template <int VW, int XMODE, int CM = -1>
__global__ void __launch_bounds__(kBlock)
k_agg_expr(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, PlanView plan,
           int use_plan, int64_t chunk, const ExprArgs ex, float* __restrict__ y, int64_t ldy,
           float* __restrict__ partial, int F) {
  constexpr int NL = expr_leaves<XMODE>();
  // edges per step: the gathered operands' U * VW values each in registers
  constexpr int NG = CM >= 0 ? NL - __builtin_popcount(CM & ((1 << NL) - 1)) : NL;
  constexpr int U = VW == 4 ? 4 : (NG <= 1 ? 16 : 8);
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  const int64_t n_items = use_plan ? plan.hdr[0] : n_rows;
  if (item >= n_items) return;
  const auto [row, eb, ee, split] = work_item(indptr, plan, use_plan, item);
  const int col = lane * VW;
  const float* base[NL];
  int64_t ld[NL];
  int kind[NL];  // 0: row indices[e], 1: row e, 2: the item's row (folded into base)
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    const int md = ex_mode(ex.code, l);
    ld[l] = ex.ld[l];
    kind[l] = md == GTA_IDX_SRC ? 0 : (md == GTA_IDX_DST ? 2 : 1);
    base[l] = ex.p[l] + col + (md == GTA_IDX_DST ? row * ld[l] : 0);
  }
  float acc[VW];
#pragma unroll
  for (int k = 0; k < VW; ++k) acc[k] = 0.f;
  // row-constant operands (the item's row, a broadcast row): loaded once, not per edge -- each
  // 64-lane load is 4 line requests at the texture units, as many as a gathered row
  Vec<VW> cst[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    if (CM >= 0 ? ((CM >> l) & 1) : (kind[l] == 2 || ld[l] == 0)) {
      kind[l] = 2;
      cst[l].load(base[l]);
    }
  }
  int idxv = (eb < ee) ? indices[min(eb + lane, ee - 1)] : 0;
  for (int64_t e0 = eb; e0 < ee; e0 += kWave) {
    const int n = static_cast<int>(min<int64_t>(kWave, ee - e0));
    const int idxn = indices[min(e0 + kWave + lane, ee - 1)];  // prefetch next block (clamped)
    for (int s = 0; s < n; s += U) {
      float L[4][U * VW];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int jj = s + u < n ? s + u : n - 1;
        const int64_t sr = __builtin_amdgcn_readlane(idxv, jj);
#pragma unroll
        for (int l = 0; l < NL; ++l) {
          Vec<VW> q;
          if (CM >= 0 ? ((CM >> l) & 1) : kind[l] == 2) {
            q = cst[l];
          } else {
            q.load(base[l] + (kind[l] == 0 ? sr : e0 + jj) * ld[l]);
          }
#pragma unroll
          for (int k = 0; k < VW; ++k) L[l][u * VW + k] = q.v[k];
        }
      }
      float t[U * VW];
      expr_eval<XMODE, U * VW>(ex.code, L, t);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < VW; ++k) acc[k] += (s + u < n) ? t[u * VW + k] : 0.f;
    }
    idxv = idxn;
  }
  Vec<VW> o;
#pragma unroll
  for (int k = 0; k < VW; ++k) o.v[k] = acc[k];
  o.store(split ? partial + item * static_cast<int64_t>(F) + col : y + row * ldy + col);
}

// Single-launch column-blocked form: one wave per plan item (a bounded part of one
// (block, row) segment), items block-major, so the waves in flight at any moment
// gather from one or two X slices.  Item k writes its partial to slab row k;
// k_seg_reduce sums each row's slab rows in (block, part) order (deterministic, no
// atomics).
template <int VW, int GL>
__global__ void __launch_bounds__(kBlock)
k_agg_seg2d(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p,
            const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, int64_t ldw,
            float* __restrict__ slabs, const SegItem* __restrict__ items) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (k >= *n_items_p) return;
  const SegItem it = items[k];
  if (it.len == 0) return;
  float acc[VW];
  lean_gather_sum<VW, GL>(indices, it.beg, it.beg + it.len, x, ldx, w, ldw, lane, acc);
  Vec<VW> o;
#pragma unroll
  for (int q = 0; q < VW; ++q) o.v[q] = acc[q];
  o.store(slabs + k * (kWave * VW) + lane * VW);
}

// Quarter-wave form of k_agg_seg2d: a wave runs FOUR consecutive (block, row) items,
// 16 lanes each (lane covers VW = F/16 floats as float4s), so one wave instruction
// gathers four source rows and the per-item start-up (record, index and first
// gather round trips, slab store) is shared by four items.  Within a 16-lane
// group the chunk's 16 source indices arrive in one coalesced load and are
// broadcast lane by lane with ds_swizzle (pattern fixed per unrolled step); lanes
// of a finished item are masked off and issue no loads.
template <int G>
__device__ __forceinline__ int bcastG(int v, int k) {  // lane k of each G-lane group (G = 16 or 32), k < G
  static_assert(G == 16 || G == 32, "group of 16 or 32 lanes");
  switch (k) {
#define GTA_BG(K_) case K_: return __builtin_amdgcn_ds_swizzle(v, (0x1F & ~(G - 1)) | (((K_) % G) << 5));
    GTA_BG(0) GTA_BG(1) GTA_BG(2) GTA_BG(3) GTA_BG(4) GTA_BG(5) GTA_BG(6) GTA_BG(7)
    GTA_BG(8) GTA_BG(9) GTA_BG(10) GTA_BG(11) GTA_BG(12) GTA_BG(13) GTA_BG(14) GTA_BG(15)
    GTA_BG(16) GTA_BG(17) GTA_BG(18) GTA_BG(19) GTA_BG(20) GTA_BG(21) GTA_BG(22) GTA_BG(23)
    GTA_BG(24) GTA_BG(25) GTA_BG(26) GTA_BG(27) GTA_BG(28) GTA_BG(29) GTA_BG(30) GTA_BG(31)
#undef GTA_BG
  }
  return v;
}

__device__ __forceinline__ int bcast16(int v, int k) {  // lane (l & 0x30) | k, k in [0, 16)
  switch (k) {
#define GTA_B16(K_) case K_: return __builtin_amdgcn_ds_swizzle(v, 0x10 | ((K_) << 5));
    GTA_B16(0) GTA_B16(1) GTA_B16(2) GTA_B16(3) GTA_B16(4) GTA_B16(5) GTA_B16(6) GTA_B16(7)
    GTA_B16(8) GTA_B16(9) GTA_B16(10) GTA_B16(11) GTA_B16(12) GTA_B16(13) GTA_B16(14) GTA_B16(15)
#undef GTA_B16
  }
  return v;
}

// Shifted softmax (gta.h, ABI 15 additive): for the exp-form score functions sf = exp . g the
// weight is v = expf(g(a + b) - m), m = the row's largest g(a + b) (k_softmax_shift), so v <= 1.
// sf_g is the value sf_apply hands to expf; sf_shift subtracts once in fp32 (never contracted
// with g's multiply) and exponentiates.
inline bool sf_is_exp_form(int sf) { return sf == GTA_SF_EXP_LEAKY_RELU || sf == GTA_SF_EXP; }
__device__ __forceinline__ float sf_g(int sf, float t) { return sf == GTA_SF_EXP ? t : (t > 0.f ? t : 0.2f * t); }
__device__ __forceinline__ float sf_shift(int sf, float t, float m) {
#pragma clang fp contract(off)
  const float g = sf_g(sf, t);
  return expf(g - m);
}

// ATT (fused GAT attention, GAT ops 6-12 minus the final SF): the edge weight is
// not read but computed, v = sf(a[row, h] + b[src, h]) from the two score tables
// (b gathered like x, from the same column block), and the item's per-head sum of
// v follows its partials in the slab row; k_seg_reduce_att divides.  No [E, H] tensor is
// written or read.
struct AttArgs {
  const float* a;  // [n_rows, H] destination-side scores (lda)
  int64_t lda;
  const float* b;  // [n_cols, H] source-side scores (ldb)
  int64_t ldb;
  int sf;
  int H;           // the item's per-head sums of v follow its F partials in the slab row (stride F + H padded to 4)
  const float* shift = nullptr;  // SH: [n_rows, H] contiguous row maxima of g(a + b) (k_softmax_shift)
};

// BF forms of the blocked item kernels (gta_aggregate_blocked_x / gta_gat_aggregate_blocked_x with
// GTA_BF16): x points at bf16 rows (read as uint16_t; ldx / row_bytes in its units) and four
// consecutive columns of a gathered row stay two raw dwords (Row4<true>) until the fma, where each
// element widens exactly (bits << 16).  Same lanes, columns, edge order and fma chain as the fp32
// form: bitwise its result on the widened table.
template <bool BF> struct Row4 {
  typedef float4 type;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <> struct Row4<true> {
  typedef uint2 type;
  static __device__ __forceinline__ uint2 zero() { return make_uint2(0u, 0u); }
};
// keeps a row piece's registers written where the source writes them (no code)
__device__ __forceinline__ void row4_pin(float4& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }
__device__ __forceinline__ void row4_pin(uint2& r) { asm volatile("" : "+v"(r.x), "+v"(r.y)); }
__device__ __forceinline__ float4 row4_f32(const float4& r) { return r; }
__device__ __forceinline__ float4 row4_f32(const uint2& r) {
  return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                     __uint_as_float(r.y & 0xffff0000u));
}

// ---- what the blocked item kernels share: item decode, row loads, slab-row store, the fold ----

// The wave's items: G lanes each (16: four per wave, 32: two), lane group j takes item
// (wave id) * (64 / G) + j; a group past n_items holds an empty item.  maxlen is the wave's longest
// item (wave-uniform), minlen (G = 32 only, where it is one more min on the same exchanged length)
// the shorter of its two.  One function for both widths: at G = 32 the butterfly is the single
// __shfl_xor the half-wave kernels always had, and a caller that does not read minlen drops it.
struct ItemSlot {
  int64_t k;  // item id = slab row
  SegItem it;
  int maxlen, minlen;
};
template <int G>
__device__ __forceinline__ ItemSlot item_decode(const int64_t* n_items_p, const SegItem* items,
                                                int lane) {
  ItemSlot d;
  d.k = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform()) * (kWave / G) + lane / G;
  const int64_t n_items = *n_items_p;
  d.it = SegItem{0, 0, 0};
  if (d.k < n_items) d.it = items[d.k];
  const int len = d.it.len;
  if constexpr (G == 32) {
    const int other = __shfl_xor(len, 32);
    d.maxlen = __builtin_amdgcn_readfirstlane(max(len, other));
    d.minlen = __builtin_amdgcn_readfirstlane(min(len, other));
  } else {
    int mx = len;
#pragma unroll
    for (int off = G; off < kWave; off <<= 1) mx = max(mx, __shfl_xor(mx, off));
    d.maxlen = __builtin_amdgcn_readfirstlane(mx);
    d.minlen = 0;
  }
  return d;
}

// Lean addressing (the half-wave kernels): row src of a table as the uniform base plus a 32-bit
// byte offset src * row_bytes + off (v_mul_u32_u24; the host checks lean32_ok), so the load takes
// the SGPR-base + VGPR-offset form.  T: the lane's piece, Row4<BF>::type of an x row or one score.
template <class T>
__device__ __forceinline__ T lean_at(const char* base, int src, uint32_t row_bytes, uint32_t off) {
  return *reinterpret_cast<const T*>(base + (__umul24(static_cast<uint32_t>(src), row_bytes) + off));
}

// Generic addressing (64-bit): the lane's NQ pieces of row src from column col.  bf16: one 8-B load
// (NQ = 1) or 16-B loads split into two pieces each (NQ = 4).
template <bool BF, int NQ>
__device__ __forceinline__ void row_load(const float* x, int64_t ldx, int src, int col,
                                         typename Row4<BF>::type (&xv)[NQ]) {
  if constexpr (BF) {
    const uint16_t* pb = reinterpret_cast<const uint16_t*>(x) + static_cast<int64_t>(src) * ldx + col;
    if constexpr (NQ % 2 == 0) {
#pragma unroll
      for (int q = 0; q < NQ; q += 2) {
        const uint4 t = reinterpret_cast<const uint4*>(pb)[q / 2];
        xv[q] = make_uint2(t.x, t.y);
        xv[q + 1] = make_uint2(t.z, t.w);
      }
    } else {
#pragma unroll
      for (int q = 0; q < NQ; ++q) xv[q] = reinterpret_cast<const uint2*>(pb)[q];
    }
  } else {
    const float4* p = reinterpret_cast<const float4*>(x + static_cast<int64_t>(src) * ldx + col);
#pragma unroll
    for (int q = 0; q < NQ; ++q) xv[q] = p[q];
  }
}

// The lane's VW partials to its slab row (NTS: non-temporal, the row is read once by the reduce)
template <bool NTS, int VW>
__device__ __forceinline__ void slab_store(float* o, const float (&acc)[VW]) {
#pragma unroll
  for (int q = 0; q < VW; ++q) {
    if (NTS) __builtin_nontemporal_store(acc[q], o + q);
    else o[q] = acc[q];
  }
}

// The fold of the unweighted item walks and of the ordered reduce: the accumulator's start value,
// the row piece an idle edge slot holds, and the per-element combine.
// FoldSum: 0, zeros, acc + x.
// FoldMax (gta_reduce_blocked's MAX / MIN): a max cannot ride on the sum's `valid ? t : 0`, so the
// accumulators start at the identity -inf, every value is flipped by the wave-uniform sign bit on
// its way in (MIN = -max(-x), exact, one instantiation for both) and an idle slot holds the
// identity -- as the bit pattern that the flip turns into -inf (RedIdle), so the fold needs no
// per-edge select and masked lanes issue no loads.  Slab rows hold partials in the MAX domain: the
// ordered reduce folds them with sbit 0 and flips the result back.
template <bool BF> struct RedIdle {  // the row piece whose every element flips to -inf
  static __device__ __forceinline__ float4 make(uint32_t sbit) {
    const float v = __uint_as_float(0xff800000u ^ sbit);
    return make_float4(v, v, v, v);
  }
};
template <> struct RedIdle<true> {
  static __device__ __forceinline__ uint2 make(uint32_t sbit) {
    const uint32_t h = (0xff800000u ^ sbit) >> 16, v = h | (h << 16);
    return make_uint2(v, v);
  }
};
template <bool BF> struct FoldSum {
  static constexpr float kInit = 0.f;
  __device__ __forceinline__ typename Row4<BF>::type idle() const { return Row4<BF>::zero(); }
  __device__ __forceinline__ float combine(float acc, float x) const { return acc + x; }
};
template <bool BF> struct FoldMax {
  uint32_t sbit;
  static constexpr float kInit = -__builtin_inff();
  __device__ __forceinline__ typename Row4<BF>::type idle() const { return RedIdle<BF>::make(sbit); }
  __device__ __forceinline__ float combine(float acc, float x) const { return red_max(acc, red_flip(x, sbit)); }
};

// The unweighted walk of a G-lane item (k_agg_seg4 without weights, k_red_seg4): a chunk's G source
// indices arrive in one coalesced load (the next chunk's behind it) and are broadcast lane by lane;
// per step U rows are gathered, lanes of a finished item masked off, and folded.  An item without
// edges, or a lane group past n_items, stores nothing.  NT as in k_agg_seg4.
template <int VW, int U, int G, int NT, bool BF, class Fold>
__device__ __forceinline__ void seg4_walk(const int32_t* indices, const int64_t* n_items_p,
                                          const float* x, int64_t ldx, float* slabs,
                                          const SegItem* items, Fold fold) {
  constexpr int F = G * VW;
  constexpr int NQ = VW / 4;
  typedef typename Row4<BF>::type XR;
  const int lane = threadIdx.x & (kWave - 1);
  const int l16 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int len = d.it.len, maxlen = d.maxlen;
  if (maxlen == 0) return;
  const int64_t eb = d.it.beg;
  const int col = l16 * VW;
  const XR idle = fold.idle();
  float acc[VW];
#pragma unroll
  for (int q = 0; q < VW; ++q) acc[q] = Fold::kInit;
  auto ldi = [&](int64_t e) { return (NT & 1) ? __builtin_nontemporal_load(indices + e) : indices[e]; };
  int idxv = (l16 < len) ? ldi(eb + l16) : 0;
  for (int c = 0; c < maxlen; c += G) {
    const int idxn = (c + G + l16 < len) ? ldi(eb + c + G + l16) : 0;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      XR xv[U][NQ];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = bcastG<G>(idxv, s + u);
        if (c + s + u < len) {
          row_load<BF, NQ>(x, ldx, src, col, xv[u]);
        } else {
#pragma unroll
          for (int q = 0; q < NQ; ++q) xv[u][q] = idle;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float4 xw = row4_f32(xv[u][q]);
          const float* xf = reinterpret_cast<const float*>(&xw);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[4 * q + t] = fold.combine(acc[4 * q + t], xf[t]);
        }
      }
    }
    idxv = idxn;
  }
  if (len > 0) slab_store<(NT & 2) != 0>(slabs + d.k * F + col, acc);
}

template <int VW, int U, bool WEIGHTED, int NT = 0, bool ATT = false, int SFC = -1, int G = 16, bool SH = false,
          bool BF = false>
// NT bit 0: non-temporal index/weight loads, bit 1: slab stores; SFC >= 0: the ATT special function
// fixed at compile time (-1: att.sf at run time); G = lanes per item (16: four items per wave,
// 32: two items per wave -- one 512-B row per half-wave instruction at F = 128); SH: the ATT
// weight is the shifted one, expf(g(a + b) - att.shift[row, h])
__global__ void __launch_bounds__(kBlock)
k_agg_seg4(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
           int64_t ldx, const float* __restrict__ w, int64_t ldw, int lph, float* __restrict__ slabs,
           const SegItem* __restrict__ items, AttArgs att = AttArgs{}) {
  if constexpr (!WEIGHTED && !ATT) {  // the plain sum: the shared walk
    seg4_walk<VW, U, G, NT, BF>(indices, n_items_p, x, ldx, slabs, items, FoldSum<BF>{});
    return;
  }
  constexpr int F = G * VW;
  constexpr int NQ = VW / 4;
  const int lane = threadIdx.x & (kWave - 1);
  const int l16 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int64_t k = d.k;
  const SegItem it = d.it;
  const int len = it.len, maxlen = d.maxlen;
  if (maxlen == 0) return;
  const int64_t eb = it.beg;
  const int col = l16 * VW;
  const int head = l16 / lph;
  float acc[VW];
#pragma unroll
  for (int q = 0; q < VW; ++q) acc[q] = 0.f;
  float arow = 0.f, ssum = 0.f;
  if (ATT && len > 0) arow = att.a[static_cast<int64_t>(it.row) * att.lda + head];
  float mrow = 0.f;
  if (ATT && SH && len > 0) mrow = att.shift[static_cast<int64_t>(it.row) * att.H + head];
  auto ldi = [&](int64_t e) { return (NT & 1) ? __builtin_nontemporal_load(indices + e) : indices[e]; };
  int idxv = (l16 < len) ? ldi(eb + l16) : 0;
  for (int c = 0; c < maxlen; c += G) {
    const int idxn = (c + G + l16 < len) ? ldi(eb + c + G + l16) : 0;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      typename Row4<BF>::type xv[U][NQ];
      float wu[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int src = bcastG<G>(idxv, s + u);
        const bool ok = c + s + u < len;
        if (ok) {
          row_load<BF, NQ>(x, ldx, src, col, xv[u]);
          if (ATT) {
            const float sv = arow + att.b[static_cast<int64_t>(src) * att.ldb + head];
            if (SH) wu[u] = (SFC >= 0) ? sf_shift(SFC, sv, mrow) : sf_shift(att.sf, sv, mrow);
            else wu[u] = (SFC >= 0) ? sf_apply(SFC, sv) : sf_apply(att.sf, sv);
            ssum += wu[u];
          } else {
            const float* wp = w + (eb + c + s + u) * ldw + head;
            wu[u] = (NT & 1) ? __builtin_nontemporal_load(wp) : *wp;
          }
        } else {
#pragma unroll
          for (int q = 0; q < NQ; ++q) xv[u][q] = Row4<BF>::zero();
          wu[u] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float4 xw = row4_f32(xv[u][q]);
          const float* xf = reinterpret_cast<const float*>(&xw);
#pragma unroll
          for (int t = 0; t < 4; ++t) acc[4 * q + t] = fmaf(wu[u], xf[t], acc[4 * q + t]);
        }
      }
    }
    idxv = idxn;
  }
  if (len > 0) {
    const int64_t lds = ATT ? F + ((att.H + 3) & ~3) : F;  // sums padded to 16 B
    slab_store<(NT & 2) != 0>(slabs + k * lds + col, acc);
    if (ATT && l16 % lph == 0) slabs[k * lds + F + head] = ssum;
  }
}

// Lean half-wave form of k_agg_seg4 for F = 128 fp32 (the metric shape): two items
// per wave, 32 lanes x float4 each, 8 edges per step.  What it removes from the
// per-edge instruction stream of the generic form:
//  * 64-bit address arithmetic: a source row is addressed as the uniform base x plus
//    a 32-bit byte offset src * row_bytes (v_mul_u32_u24; the host checks the
//    gathered table spans < 2^32 bytes and n_cols < 2^24), so the load takes the
//    SGPR-base + VGPR-offset form;
//  * per-edge exec masking: a step where BOTH items still hold 8 edges (wave-uniform
//    test against the shorter item) runs unmasked; only the tail steps are masked;
//  * per-edge weight loads (8 heads, 4 lanes per head, WEIGHTED): lane (h, q) loads
//    alpha[e + 2q][h] and alpha[e + 2q + 1][h] -- two dword loads per step -- and edge
//    u's weight reaches its head's 4 lanes by a DPP quad broadcast from quad lane u/2.
// Same per-lane edge order and fma chain as k_agg_seg4: results bitwise equal to it.
template <int SEL>
__device__ __forceinline__ float quad_bcast(float v) {  // lane (l & ~3) | SEL of each quad
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), SEL * 0x55, 0xF, 0xF, false));
}

// lane l ^ 4: the neighbouring quad of a 16-lane row.  gfx9 DPP has no row_xmask, so two row
// rotations (row_ror:n -- lane l reads lane (l - n) mod 16 of its row) and a pick by quad parity
__device__ __forceinline__ float xmask4(float v, bool odd_quad) {
  const float from_lo = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xF, 0xF, false));
  const float from_hi = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x12C, 0xF, 0xF, false));
  return odd_quad ? from_lo : from_hi;
}

// W1 (WEIGHTED with one weight per edge, e.g. GCN / GraphSAGE-mean [E, 1]): the weights of a
// 32-edge chunk arrive with its indices (lane l loads w[e + l]) and edge u's weight is broadcast
// like its index (bcastG), instead of one load per edge per lane.
// A1 (8 heads, ldw even, 8-B aligned weights): a full step's 8 x 8 weights arrive in ONE 8-B load
// per lane instead of two 4-B loads: lane (h, q) loads heads 2(h/2), 2(h/2)+1 of edge 2q + h%2, so
// the quad of head h holds head h's weights of edges 2k + h%2 (k = quad lane) and the neighbouring
// quad (h ^ 1, two DPP row rotations away) those of edges 2k + (h^1)%2; each edge's weight then
// reaches the head's lanes by the same quad broadcasts, picked per lane by head parity.  The same
// weights enter the same fma chain: bitwise equal to the two-load form.  (the alpha
// loads were ~19 % of the kernel's vector-memory instructions; the texture path is its bound.)
// BF: bf16 rows in the same lane layout with half-width loads -- 32 lanes x 8 B, one 256-B row per
// half-wave instruction (row_bytes = 2 ldx; the host guards are restated for 2-byte elements).
// The unweighted lean walk (k_agg_h32 without weights, k_red_h32): seg4_walk's chunks and steps at
// G = 32, U = 8 with lean row addressing and the full / tail split.  NT bit 0: non-temporal index
// loads, bit 1: non-temporal slab stores.
template <int NT, bool BF, class Fold>
__device__ __forceinline__ void h32_walk(const int32_t* indices, const int64_t* n_items_p,
                                         const float* x, uint32_t row_bytes, float* slabs,
                                         const SegItem* items, Fold fold) {
  constexpr int G = 32, F = 128, U = 8;
  typedef typename Row4<BF>::type XR;
  const int lane = threadIdx.x & (kWave - 1);
  const int l32 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int len = d.it.len, maxlen = d.maxlen, minlen = d.minlen;
  if (maxlen == 0) return;
  const uint32_t colb = static_cast<uint32_t>(l32) * (BF ? 8u : 16u);
  const char* xb = reinterpret_cast<const char*>(x);
  const int32_t* ic = indices + d.it.beg;  // chunk cursor: advanced once per 32 edges
  const XR idle = fold.idle();
  float acc[4] = {Fold::kInit, Fold::kInit, Fold::kInit, Fold::kInit};
  auto ldi = [&](const int32_t* p) { return (NT & 1) ? __builtin_nontemporal_load(p) : *p; };
  int idxv = (l32 < len) ? ldi(ic + l32) : 0;
  for (int c = 0; c < maxlen; c += G) {
    const int idxn = (c + G + l32 < len) ? ldi(ic + G + l32) : 0;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      XR xv[U];
      if (c + s + U <= minlen) {  // full step for both items: no masks
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = lean_at<XR>(xb, bcastG<G>(idxv, s + u), row_bytes, colb);
      } else {
        const int rem = len - c - s;  // edges of this item left at this step (may be <= 0)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = bcastG<G>(idxv, s + u);
          if (u < rem) xv[u] = lean_at<XR>(xb, src, row_bytes, colb);
          else xv[u] = idle;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 xw = row4_f32(xv[u]);
        acc[0] = fold.combine(acc[0], xw.x);
        acc[1] = fold.combine(acc[1], xw.y);
        acc[2] = fold.combine(acc[2], xw.z);
        acc[3] = fold.combine(acc[3], xw.w);
      }
    }
    idxv = idxn;
    ic += G;
  }
  if (len > 0) slab_store<(NT & 2) != 0>(slabs + d.k * F + l32 * 4, acc);
}

// A1: a step's weights from the lane's one 8-B load pr (odd: the lane's head is odd) -- wu[u] is
// edge u's weight of the lane's head
__device__ __forceinline__ void a1_spread(const float2 pr, const bool odd, float (&wu)[8]) {
  const float own = odd ? pr.y : pr.x, oth = xmask4(odd ? pr.x : pr.y, odd);
  float a[4], b[4];
  a[0] = quad_bcast<0>(own); b[0] = quad_bcast<0>(oth);
  a[1] = quad_bcast<1>(own); b[1] = quad_bcast<1>(oth);
  a[2] = quad_bcast<2>(own); b[2] = quad_bcast<2>(oth);
  a[3] = quad_bcast<3>(own); b[3] = quad_bcast<3>(oth);
#pragma unroll
  for (int k2 = 0; k2 < 4; ++k2) {
    wu[2 * k2] = odd ? b[k2] : a[k2];
    wu[2 * k2 + 1] = odd ? a[k2] : b[k2];
  }
}

// GR (A1 with ldw == 8, weights and indices 128-B aligned; knob seg_grid): the A1 walk with its
// steps on the global edge grid instead of at the item's first edge.  An item [beg, beg + len)
// walks the aligned 8-edge windows from beg & ~7, so a step's 8 x 8 weights are exactly two 128-B
// lines (2.75 on average from an arbitrary beg) and the first and last steps mask the edges
// outside the item: those lanes load no weight (w = +0 through the DPP spread) and gather no row
// (x = 0), as the tail steps of the walk above.  The indices come by aligned 32-edge chunks, one
// line per load: lane l holds entry (l + r) & 31 of its chunk, r = beg & 24, so lanes l < 32 - r
// of chunk m and l >= 32 - r of chunk m + 1 together are the 32 edges from (beg & ~7) + 32 m in
// lane order -- one select per 32 edges, then the walk's fixed broadcasts.  Items are clamped to
// nnz: no index or weight outside [0, nnz) is read.  Same per-lane edge order and fma chain as
// the A1 form: bitwise equal to it.
template <int NT, bool BF>
__device__ __forceinline__ void h32_grid_walk(const int32_t* indices, const int64_t* n_items_p,
                                              const float* x, uint32_t row_bytes, const float* w,
                                              uint32_t nnz, float* slabs, const SegItem* items) {
  constexpr int G = 32, F = 128, U = 8;
  typedef typename Row4<BF>::type XR;
  const int lane = threadIdx.x & (kWave - 1);
  const int l32 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const uint32_t beg = static_cast<uint32_t>(d.it.beg);  // host: nnz * 32 < 2^32
  const uint32_t last = min(beg + static_cast<uint32_t>(max(d.it.len, 0)), nnz);
  const uint32_t len = last > beg ? last - beg : 0u;
  const uint32_t end = len ? last : 0u;  // an empty item loads nothing
  const int f = len ? static_cast<int>(beg & 7u) : 0;  // edges of the first window before the item
  const int glen = len ? f + static_cast<int>(len) : 0;  // the item's end, counted from beg & ~7
  const int other = __shfl_xor(glen, 32);
  const int gmax = __builtin_amdgcn_readfirstlane(max(glen, other));
  const int gmin = __builtin_amdgcn_readfirstlane(min(glen, other));
  if (gmax == 0) return;
  const bool front = __ballot(f != 0) != 0;  // some item of the wave starts inside its first window
  const uint32_t colb = static_cast<uint32_t>(l32) * (BF ? 8u : 16u);
  const char* xb = reinterpret_cast<const char*>(x);
  const int h = l32 >> 2, q = l32 & 3;
  const bool odd = h & 1;
  const int wl = 2 * q + (h & 1);  // the window's edge whose weights this lane loads (heads h & ~1, h | 1)
  const char* wbase = reinterpret_cast<const char*>(w);
  uint32_t woff = (((beg & ~7u) + static_cast<uint32_t>(wl)) * 8u + static_cast<uint32_t>(h & ~1)) * 4u;
  const char* ibase = reinterpret_cast<const char*>(indices);
  const uint32_t r = beg & 24u;
  const bool lo = static_cast<uint32_t>(l32) + r < 32u;
  uint32_t ie = (beg & ~31u) + ((static_cast<uint32_t>(l32) + r) & 31u);  // the lane's entry of the chunk
  auto ldc = [&](uint32_t e) {  // a chunk's entry, where the item needs it
    if (e >= end) return 0;
    const int32_t* p = reinterpret_cast<const int32_t*>(ibase + (e << 2));
    return (NT & 1) ? __builtin_nontemporal_load(p) : *p;
  };
  auto wld = [&](uint32_t off) { return *reinterpret_cast<const float2*>(wbase + off); };
  auto row = [&](int src) { return lean_at<XR>(xb, src, row_bytes, colb); };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int i0 = ldc(ie);
  int in = ldc(ie + G);
  int idxv = lo ? i0 : in;  // the 32 edges from beg & ~7, lane = edge
  ie += 2 * G;
  for (int c = 0; c < gmax; c += G) {
    const int inn = ldc(ie);  // two chunks ahead: the next 32 edges end in it
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= gmax) break;
      XR xv[U];
      float wu[U];
      if (c + s + U <= gmin && (s > 0 || c > 0 || !front)) {  // inside both items: no masks
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = row(bcastG<G>(idxv, s + u));
        a1_spread(wld(woff + static_cast<uint32_t>(s) * 32u), odd, wu);
      } else {
        const int p = c + s - f;  // the window's first edge, counted from beg (may be < 0)
        // the masked rows' zeros are written here, before any load of the step is issued: written
        // edge by edge between the gathers, each write waited for the loads issued before it
#pragma unroll
        for (int u = 0; u < U; ++u) {
          xv[u] = Row4<BF>::zero();
          row4_pin(xv[u]);
        }
        float2 pr = make_float2(0.f, 0.f);
        if (static_cast<uint32_t>(p + wl) < len) pr = wld(woff + static_cast<uint32_t>(s) * 32u);
        int src[U];  // the eight broadcasts back to back, ahead of the masked gathers
#pragma unroll
        for (int u = 0; u < U; ++u) src[u] = bcastG<G>(idxv, s + u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (static_cast<uint32_t>(p + u) < len) xv[u] = row(src[u]);
        }
        a1_spread(pr, odd, wu);  // after the gathers are issued; an edge outside the item: no lane loaded it, w = +0
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 xw = row4_f32(xv[u]);
        acc[0] = fmaf(wu[u], xw.x, acc[0]);
        acc[1] = fmaf(wu[u], xw.y, acc[1]);
        acc[2] = fmaf(wu[u], xw.z, acc[2]);
        acc[3] = fmaf(wu[u], xw.w, acc[3]);
      }
    }
    idxv = lo ? in : inn;
    in = inn;
    ie += G;
    woff += static_cast<uint32_t>(G) * 32u;
  }
  if (len) slab_store<(NT & 2) != 0>(slabs + d.k * F + l32 * 4, acc);
}

template <bool WEIGHTED, int NT, bool W1 = false, bool A1 = false, bool BF = false, bool GR = false>
__global__ void __launch_bounds__(kBlock)
k_agg_h32(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
          uint32_t row_bytes, const float* __restrict__ w, int64_t ldw, float* __restrict__ slabs,
          const SegItem* __restrict__ items, uint32_t nnz = 0) {
  if constexpr (!WEIGHTED) {  // the plain sum: the shared walk
    h32_walk<NT, BF>(indices, n_items_p, x, row_bytes, slabs, items, FoldSum<BF>{});
    return;
  }
  if constexpr (GR) {  // the A1 walk on the edge grid
    static_assert(WEIGHTED && A1 && !W1, "the grid walk is a form of A1");
    h32_grid_walk<NT, BF>(indices, n_items_p, x, row_bytes, w, nnz, slabs, items);
    return;
  }
  constexpr int G = 32, F = 128, U = 8;
  const int lane = threadIdx.x & (kWave - 1);
  const int l32 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int64_t k = d.k;
  const SegItem it = d.it;
  const int len = it.len, maxlen = d.maxlen, minlen = d.minlen;
  if (maxlen == 0) return;
  typedef typename Row4<BF>::type XR;
  const uint32_t colb = static_cast<uint32_t>(l32) * (BF ? 8u : 16u);
  const char* xb = reinterpret_cast<const char*>(x);
  const int h = l32 >> 2, q = l32 & 3;
  const int ldw32 = static_cast<int>(ldw);
  // chunk cursors: advanced once per 32 edges, so no per-edge 64-bit offsets are live
  const int32_t* ic = indices + it.beg;
  const float* wc = !A1 ? w + it.beg * ldw + (W1 ? 0 : h) : nullptr;
  // A1: the weights as the uniform base w + a 32-bit byte offset (host: nnz * ldw * 4 < 2^32), like
  // the rows -- with 64-bit per-lane pointers the compiler strength-reduced every (step, edge)
  // weight address into its own 64-bit induction variable (134 VGPRs, 3 waves per SIMD)
  const char* wbase = reinterpret_cast<const char*>(w);
  uint32_t woff = A1 ? static_cast<uint32_t>((it.beg * ldw + h) * 4) : 0u;
  const uint32_t wrow = static_cast<uint32_t>(ldw) * 4u;
  auto wat = [&](uint32_t off) { return *reinterpret_cast<const float*>(wbase + off); };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  // NT bit 0: non-temporal index loads, bit 2: non-temporal weight loads (both streams are read
  // once), bit 1: non-temporal slab stores
  auto ldi = [&](const int32_t* p) { return (NT & 1) ? __builtin_nontemporal_load(p) : *p; };
  auto ldw_ = [&](const float* p) { return (NT & 4) ? __builtin_nontemporal_load(p) : *p; };
  auto row = [&](int src) { return lean_at<XR>(xb, src, row_bytes, colb); };
  int idxv = (l32 < len) ? ldi(ic + l32) : 0;
  float wv = (W1 && l32 < len) ? ldw_(wc + l32 * ldw32) : 0.f;  // W1: this chunk's weights, lane = edge
  for (int c = 0; c < maxlen; c += G) {
    const int idxn = (c + G + l32 < len) ? ldi(ic + G + l32) : 0;
    const float wvn = (W1 && c + G + l32 < len) ? ldw_(wc + (G + l32) * ldw32) : 0.f;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      XR xv[U];
      float wu[U];
      if (c + s + U <= minlen) {  // full step for both items: no masks
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = row(bcastG<G>(idxv, s + u));
        if (W1) {
#pragma unroll
          for (int u = 0; u < U; ++u) wu[u] = __int_as_float(bcastG<G>(__float_as_int(wv), s + u));
        } else if (A1) {
          const float2 pr = *reinterpret_cast<const float2*>(
              wbase + (woff + static_cast<uint32_t>((h & 1) + s + 2 * q) * wrow + static_cast<uint32_t>(2 * (h >> 1) - h) * 4u));
          a1_spread(pr, h & 1, wu);
        } else {
          const float* wp = wc + (s + 2 * q) * ldw32;
          const float w0 = ldw_(wp), w1 = ldw_(wp + ldw32);
          wu[0] = quad_bcast<0>(w0); wu[1] = quad_bcast<0>(w1);
          wu[2] = quad_bcast<1>(w0); wu[3] = quad_bcast<1>(w1);
          wu[4] = quad_bcast<2>(w0); wu[5] = quad_bcast<2>(w1);
          wu[6] = quad_bcast<3>(w0); wu[7] = quad_bcast<3>(w1);
        }
      } else {
        const int rem = len - c - s;  // edges of this item left at this step (may be <= 0)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = bcastG<G>(idxv, s + u);
          if (u < rem) {
            xv[u] = row(src);
            wu[u] = W1 ? __int_as_float(bcastG<G>(__float_as_int(wv), s + u))
                       : (A1 ? wat(woff + static_cast<uint32_t>(s + u) * wrow) : ldw_(wc + (s + u) * ldw32));
          } else {
            xv[u] = Row4<BF>::zero();
            wu[u] = 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 xw = row4_f32(xv[u]);
        acc[0] = fmaf(wu[u], xw.x, acc[0]);
        acc[1] = fmaf(wu[u], xw.y, acc[1]);
        acc[2] = fmaf(wu[u], xw.z, acc[2]);
        acc[3] = fmaf(wu[u], xw.w, acc[3]);
      }
    }
    idxv = idxn;
    if (W1) wv = wvn;
    ic += G;
    if (A1) woff += static_cast<uint32_t>(G) * wrow;
    else wc += static_cast<int64_t>(G) * ldw;
  }
  if (len > 0) slab_store<(NT & 2) != 0>(slabs + k * F + l32 * 4, acc);
}

// Column-blocked MAX / MIN (gta_reduce_blocked): the unweighted walks with FoldMax.  Item k's slab
// row holds its partial in the MAX domain; k_seg_reduce_red folds and flips back.
// k_red_seg4: G = 16 for F = 64 / 256 (four items per wave), G = 32 for F = 128 (two; non-temporal
// slab stores).  k_red_h32: the lean F = 128 form.
template <int VW, int U, int G, bool BF>
__global__ void __launch_bounds__(kBlock)
k_red_seg4(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
           int64_t ldx, uint32_t sbit, float* __restrict__ slabs, const SegItem* __restrict__ items) {
  seg4_walk<VW, U, G, (G == 32 ? 2 : 0), BF>(indices, n_items_p, x, ldx, slabs, items, FoldMax<BF>{sbit});
}

template <int NT, bool BF>
__global__ void __launch_bounds__(kBlock)
k_red_h32(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
          uint32_t row_bytes, uint32_t sbit, float* __restrict__ slabs, const SegItem* __restrict__ items) {
  h32_walk<NT, BF>(indices, n_items_p, x, row_bytes, slabs, items, FoldMax<BF>{sbit});
}

// Round 6: the metric kernel with its two streamed inputs -- alpha (32 B per edge) and the source
// indices (4 B) -- pre-fetched into L2 by SCALAR loads (knob seg_pf; k_agg_h32<A1> otherwise).
// Why: counters of k_agg_h32 (profiles/r05/wcost_pmc_summary.json) put the kernel's limit in the
// vector L1's outstanding-request capacity: ~90 line requests in flight per CU, so throughput =
// capacity / mean latency.  The alpha lines are all HBM misses (~1,800 cycles each against ~360
// for the gathered rows, 70 % L2 hits) and hold a third of that capacity: without alpha the
// same loop runs in 0.68 of the time.  A vector prefetch cannot help -- loads return in order, so
// waiting for a step's rows waits for any earlier prefetch too -- but a scalar load is counted on
// lgkmcnt and travels the scalar cache: issued PD steps ahead it brings the alpha lines (and the
// next chunk's index line) into L2, and the vector loads then hit.  For that the loop keeps no LDS
// operation in flight (lgkmcnt would otherwise mix the two): the index of edge u reaches the
// half-wave by a DPP row broadcast (row_newbcast) from a register in which lanes j and j + 16 hold
// the same index, instead of ds_swizzle.  The prefetched values are never used; each is kept live
// until an explicit s_waitcnt lgkmcnt(0) one step later, so no register is reused while its load
// is in flight (asmcheck.py checks the built code).  s_buffer_load through a descriptor bounded
// by the tensor: a prefetch past the end reads nothing.  PFB = prefetch granule (64 or 128 B).
// Same per-lane edge order and fma chain as k_agg_h32: bitwise equal to it.
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4_t buf_desc(const void* p, uint32_t bytes) {  // raw buffer: stride 0, bounds = bytes
  const uint64_t a = reinterpret_cast<uint64_t>(p);
  return i32x4_t{static_cast<int>(a & 0xffffffffu), static_cast<int>((a >> 32) & 0xffffu), static_cast<int>(bytes),
                 0x00020000};
}
template <int K>
__device__ __forceinline__ int row_bcast(int v) {  // lane K of each 16-lane row (gfx90a+ DPP row_newbcast)
  return __builtin_amdgcn_update_dpp(0, v, 0x150 + K, 0xF, 0xF, false);
}

template <int K>
__device__ __forceinline__ int idx_bcast(int lo, int hi) {  // index K (< 32) of the chunk to the half-wave
  return K < 16 ? row_bcast<K % 16>(lo) : row_bcast<K % 16>(hi);
}

__device__ __forceinline__ void spf(int& d, const i32x4_t& rs, uint32_t off) {  // scalar L2 prefetch of one granule
  asm volatile("s_buffer_load_dword %0, %1, %2" : "=s"(d) : "s"(rs), "s"(off) : "memory");
}

template <int NT, int PFB, int PD, int MINW = 1>
__global__ void __launch_bounds__(kBlock, MINW)
k_agg_h32pf(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
            uint32_t row_bytes, const float* __restrict__ w, int64_t ldw, float* __restrict__ slabs,
            const SegItem* __restrict__ items, uint32_t w_bytes, uint32_t i_bytes) {
  constexpr int G = 32, F = 128, U = 8;
  constexpr int NPA = 256 / PFB;  // granules of one item's alpha per step (8 edges x 32 B)
  const int lane = threadIdx.x & (kWave - 1);
  const int l32 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int64_t k = d.k;
  const SegItem it = d.it;
  const int len = it.len, maxlen = d.maxlen, minlen = d.minlen;
  if (maxlen == 0) return;
  // the two items as scalars (A: lanes 0-31, B: lanes 32-63); edge ids < 2^27 (host: nnz * 32 < 2^32)
  const uint32_t begA = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(it.beg), 0));
  const uint32_t begB = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(it.beg), 32));
  const int lenA = __builtin_amdgcn_readlane(len, 0), lenB = __builtin_amdgcn_readlane(len, 32);
  const uint32_t wrow = static_cast<uint32_t>(ldw) * 4u;
  const i32x4_t rsw = buf_desc(w, w_bytes), rsi = buf_desc(indices, i_bytes);
  const uint32_t colb = static_cast<uint32_t>(l32) * 16u;
  const char* xb = reinterpret_cast<const char*>(x);
  const int h = l32 >> 2, q = l32 & 3;
  const int32_t* ic = indices + it.beg;
  const char* wbase = reinterpret_cast<const char*>(w);
  uint32_t woff = static_cast<uint32_t>((it.beg * ldw + h) * 4);
  auto wat = [&](uint32_t off) { return *reinterpret_cast<const float*>(wbase + off); };
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  auto ldi = [&](const int32_t* p) { return (NT & 1) ? __builtin_nontemporal_load(p) : *p; };
  auto row = [&](int src) { return lean_at<float4>(xb, src, row_bytes, colb); };
  // prefetch bookkeeping: the granules issued at the previous step, kept live until the next wait
  int pfa[2 * NPA], pfi[4];
#pragma unroll
  for (int j = 0; j < 2 * NPA; ++j) pfa[j] = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) pfi[j] = 0;
  auto retire = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < 2 * NPA; ++j) asm volatile("" ::"s"(pfa[j]));
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"s"(pfi[j]));
  };
  // alpha of step t (edges 8t .. 8t + 7 of each item) into L2
  auto pf_alpha = [&](int t) __attribute__((always_inline)) {
    const int e = 8 * t;
    if (e < lenA) {
      const uint32_t o = ((begA + static_cast<uint32_t>(e)) * wrow) & ~static_cast<uint32_t>(PFB - 1);
#pragma unroll
      for (int j = 0; j < NPA; ++j) spf(pfa[j], rsw, o + j * PFB);
    }
    if (e < lenB) {
      const uint32_t o = ((begB + static_cast<uint32_t>(e)) * wrow) & ~static_cast<uint32_t>(PFB - 1);
#pragma unroll
      for (int j = 0; j < NPA; ++j) spf(pfa[NPA + j], rsw, o + j * PFB);
    }
  };
  // the 128 B of indices of chunk c (32 edges) into L2
  auto pf_idx = [&](int c) __attribute__((always_inline)) {
    if (c < lenA) {
      const uint32_t o = ((begA + static_cast<uint32_t>(c)) * 4u) & ~63u;
      spf(pfi[0], rsi, o);
      spf(pfi[1], rsi, o + 64);
    }
    if (c < lenB) {
      const uint32_t o = ((begB + static_cast<uint32_t>(c)) * 4u) & ~63u;
      spf(pfi[2], rsi, o);
      spf(pfi[3], rsi, o + 64);
    }
  };
#pragma unroll
  for (int t = 1; t <= PD; ++t) pf_alpha(t);
  pf_idx(G);
  // lanes j and j + 16 of a half hold the same index: lo = index j % 16, hi = index 16 + j % 16
  const int jl = l32 & 15;
  int ilo = (jl < len) ? ldi(ic + jl) : 0;
  int ihi = (16 + jl < len) ? ldi(ic + 16 + jl) : 0;
  for (int c = 0; c < maxlen; c += G) {
    // opaque to loop strength reduction: otherwise each of the 32 (step, edge) weight offsets of a
    // chunk became its own induction register (95 VGPRs)
    asm volatile("" : "+v"(woff));
    const int ilon = (c + G + jl < len) ? ldi(ic + G + jl) : 0;
    const int ihin = (c + G + 16 + jl < len) ? ldi(ic + G + 16 + jl) : 0;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      // the previous step's prefetches have landed; issue the step PD ahead (and at a chunk's
      // first step, the indices of the chunk after the next)
      retire();
      pf_alpha((c + s) / U + PD + 1);
      if (s == 0) pf_idx(c + 2 * G);
      // keep each step's index broadcasts in the step: hoisted to the chunk start they held 32
      // more VGPRs (95: 5 waves per SIMD instead of 8)
      __builtin_amdgcn_sched_barrier(0);
      float4 xv[U];
      float wu[U];
      if (c + s + U <= minlen) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int src;
          switch (s + u) {
#define GTA_IB(K_) case K_: src = idx_bcast<K_>(ilo, ihi); break;
            GTA_IB(0) GTA_IB(1) GTA_IB(2) GTA_IB(3) GTA_IB(4) GTA_IB(5) GTA_IB(6) GTA_IB(7)
            GTA_IB(8) GTA_IB(9) GTA_IB(10) GTA_IB(11) GTA_IB(12) GTA_IB(13) GTA_IB(14) GTA_IB(15)
            GTA_IB(16) GTA_IB(17) GTA_IB(18) GTA_IB(19) GTA_IB(20) GTA_IB(21) GTA_IB(22) GTA_IB(23)
            GTA_IB(24) GTA_IB(25) GTA_IB(26) GTA_IB(27) GTA_IB(28) GTA_IB(29) GTA_IB(30) GTA_IB(31)
#undef GTA_IB
            default: src = 0;
          }
          xv[u] = row(src);
        }
        const float2 pr = *reinterpret_cast<const float2*>(
            wbase + (woff + static_cast<uint32_t>((h & 1) + s + 2 * q) * wrow + static_cast<uint32_t>(2 * (h >> 1) - h) * 4u));
        const bool odd = h & 1;
        const float own = odd ? pr.y : pr.x, oth = xmask4(odd ? pr.x : pr.y, odd);
        float a[4], b[4];
        a[0] = quad_bcast<0>(own); b[0] = quad_bcast<0>(oth);
        a[1] = quad_bcast<1>(own); b[1] = quad_bcast<1>(oth);
        a[2] = quad_bcast<2>(own); b[2] = quad_bcast<2>(oth);
        a[3] = quad_bcast<3>(own); b[3] = quad_bcast<3>(oth);
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
          wu[2 * k2] = odd ? b[k2] : a[k2];
          wu[2 * k2 + 1] = odd ? a[k2] : b[k2];
        }
      } else {
        const int rem = len - c - s;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          int src;
          switch (s + u) {
#define GTA_IB(K_) case K_: src = idx_bcast<K_>(ilo, ihi); break;
            GTA_IB(0) GTA_IB(1) GTA_IB(2) GTA_IB(3) GTA_IB(4) GTA_IB(5) GTA_IB(6) GTA_IB(7)
            GTA_IB(8) GTA_IB(9) GTA_IB(10) GTA_IB(11) GTA_IB(12) GTA_IB(13) GTA_IB(14) GTA_IB(15)
            GTA_IB(16) GTA_IB(17) GTA_IB(18) GTA_IB(19) GTA_IB(20) GTA_IB(21) GTA_IB(22) GTA_IB(23)
            GTA_IB(24) GTA_IB(25) GTA_IB(26) GTA_IB(27) GTA_IB(28) GTA_IB(29) GTA_IB(30) GTA_IB(31)
#undef GTA_IB
            default: src = 0;
          }
          if (u < rem) {
            xv[u] = row(src);
            wu[u] = wat(woff + static_cast<uint32_t>(s + u) * wrow);
          } else {
            xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            wu[u] = 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc[0] = fmaf(wu[u], xv[u].x, acc[0]);
        acc[1] = fmaf(wu[u], xv[u].y, acc[1]);
        acc[2] = fmaf(wu[u], xv[u].z, acc[2]);
        acc[3] = fmaf(wu[u], xv[u].w, acc[3]);
      }
    }
    ilo = ilon;
    ihi = ihin;
    ic += G;
    woff += static_cast<uint32_t>(G) * wrow;
  }
  retire();  // no scalar load in flight when the wave ends
  if (len > 0) slab_store<(NT & 2) != 0>(slabs + k * F + l32 * 4, acc);
}

// Lean half-wave form of the fused GAT attention item (k_agg_seg4<4, 8, ATT, SFC = exp-leaky-
// relu, G = 32>) for F = 128, 8 heads: the weighted k_agg_h32 loop with the edge weight computed,
// v = exp(leaky_relu(a[row, h] + b[src, h])), instead of loaded.  Per full 8-edge step lane
// (h, q) gathers the scores of edges 2q and 2q+1 (their sources picked from the step's
// broadcast indices by q), evaluates 2 special functions instead of 8, and edge u's v reaches the
// head's four lanes by a DPP quad broadcast, as the weights do in k_agg_h32.  Score rows are
// addressed like X rows (uniform base + 32-bit byte offset).  Same per-lane edge order, fma chain
// and per-head sum order as the generic form: bitwise equal to it.  Slab row k: 128 partials,
// then the 8 per-head sums of v.
// Direct epilogue (row_ptr given): an item that is its row's only item (low-degree rows at
// small B) writes y (and sums) itself, exactly as the ordered reduce would (0 + p = p), and the
// reduce skips its row (k_seg_reduce_att with skip_single).
// SH: the shifted weight, v = expf(leaky_relu(a + b) - shift[row, h]); the row's shift is loaded
// once beside a[row, h], the 2-SF step and the direct epilogue are unchanged.
// BF: bf16 x rows as in k_agg_h32<BF> (the score tables stay fp32).
template <int NT, bool SH = false, bool BF = false>
__global__ void __launch_bounds__(kBlock)
k_att_h32(const int32_t* __restrict__ indices, const int64_t* __restrict__ n_items_p, const float* __restrict__ x,
          uint32_t row_bytes, const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
          uint32_t brow_bytes, float* __restrict__ slabs, const SegItem* __restrict__ items,
          const int64_t* __restrict__ row_ptr = nullptr, int normalize = 1, float* __restrict__ y = nullptr,
          int64_t ldy = 0, float* __restrict__ sums = nullptr, int sf_out = GTA_SF_NONE,
          const float* __restrict__ shift = nullptr) {
  constexpr int G = 32, U = 8, F = 128, LDS = F + 8;
  const int lane = threadIdx.x & (kWave - 1);
  const int l32 = lane & (G - 1);
  const ItemSlot d = item_decode<G>(n_items_p, items, lane);
  const int64_t k = d.k;
  const SegItem it = d.it;
  const int len = it.len, maxlen = d.maxlen, minlen = d.minlen;
  if (maxlen == 0) return;
  const int h = l32 >> 2, q = l32 & 3;
  typedef typename Row4<BF>::type XR;
  const uint32_t colb = static_cast<uint32_t>(l32) * (BF ? 8u : 16u), hb = static_cast<uint32_t>(h) * 4u;
  const char* xb = reinterpret_cast<const char*>(x);
  const char* bb = reinterpret_cast<const char*>(b);
  const float arow = (len > 0) ? a[static_cast<int64_t>(it.row) * lda + h] : 0.f;
  const float mrow = (SH && len > 0) ? shift[static_cast<int64_t>(it.row) * 8 + h] : 0.f;
  auto ldi = [&](const int32_t* p) { return (NT & 1) ? __builtin_nontemporal_load(p) : *p; };
  auto row = [&](int src) { return lean_at<XR>(xb, src, row_bytes, colb); };
  auto score = [&](int src) -> float {
    const float sv = arow + lean_at<float>(bb, src, brow_bytes, hb);
    return SH ? sf_shift(GTA_SF_EXP_LEAKY_RELU, sv, mrow) : sf_apply(GTA_SF_EXP_LEAKY_RELU, sv);
  };
  const int32_t* ic = indices + it.beg;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float ssum = 0.f;
  int idxv = (l32 < len) ? ldi(ic + l32) : 0;
  for (int c = 0; c < maxlen; c += G) {
    const int idxn = (c + G + l32 < len) ? ldi(ic + G + l32) : 0;
#pragma unroll
    for (int s = 0; s < G; s += U) {
      if (c + s >= maxlen) break;
      XR xv[U];
      float wu[U];
      if (c + s + U <= minlen) {  // full step for both items: no masks
        int src[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          src[u] = bcastG<G>(idxv, s + u);
          xv[u] = row(src[u]);
        }
        const int sa = q == 0 ? src[0] : q == 1 ? src[2] : q == 2 ? src[4] : src[6];
        const int sb = q == 0 ? src[1] : q == 1 ? src[3] : q == 2 ? src[5] : src[7];
        const float v0 = score(sa), v1 = score(sb);
        wu[0] = quad_bcast<0>(v0); wu[1] = quad_bcast<0>(v1);
        wu[2] = quad_bcast<1>(v0); wu[3] = quad_bcast<1>(v1);
        wu[4] = quad_bcast<2>(v0); wu[5] = quad_bcast<2>(v1);
        wu[6] = quad_bcast<3>(v0); wu[7] = quad_bcast<3>(v1);
#pragma unroll
        for (int u = 0; u < U; ++u) ssum += wu[u];
      } else {
        const int rem = len - c - s;  // edges of this item left at this step (may be <= 0)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = bcastG<G>(idxv, s + u);
          if (u < rem) {
            xv[u] = row(src);
            wu[u] = score(src);
            ssum += wu[u];
          } else {
            xv[u] = Row4<BF>::zero();
            wu[u] = 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float4 xw = row4_f32(xv[u]);
        acc[0] = fmaf(wu[u], xw.x, acc[0]);
        acc[1] = fmaf(wu[u], xw.y, acc[1]);
        acc[2] = fmaf(wu[u], xw.z, acc[2]);
        acc[3] = fmaf(wu[u], xw.w, acc[3]);
      }
    }
    idxv = idxn;
    ic += G;
  }
  if (len > 0) {
    if (row_ptr != nullptr && row_ptr[it.row + 1] - row_ptr[it.row] == 1) {  // the row's only item
      const float sh = 0.f + ssum;
      float4 v;
      v.x = 0.f + acc[0]; v.y = 0.f + acc[1]; v.z = 0.f + acc[2]; v.w = 0.f + acc[3];
      if (normalize) {
        v.x /= sh; v.y /= sh; v.z /= sh; v.w /= sh;
      }
      if (sf_out != GTA_SF_NONE) {  // the layer's SF on y (GAT op 13), as the reduce applies it
        v.x = sf_apply(sf_out, v.x); v.y = sf_apply(sf_out, v.y); v.z = sf_apply(sf_out, v.z); v.w = sf_apply(sf_out, v.w);
      }
      *reinterpret_cast<float4*>(y + static_cast<int64_t>(it.row) * ldy + l32 * 4) = v;
      if (sums != nullptr && q == 0) sums[static_cast<int64_t>(it.row) * 8 + h] = sh;
      return;
    }
    float* o = slabs + k * LDS;
    slab_store<(NT & 2) != 0>(o + l32 * 4, acc);
    if (q == 0) o[F + h] = ssum;
  }
}

// The row's slab rows (item ids row_items[row_ptr[row] .. row_ptr[row+1]), in
// (block, part) order) summed in that order; ids arrive 64 at a time with one
// coalesced load and are broadcast by readlane, 4 slab loads in flight.
struct RowItems {
  const int64_t* row_ptr;
  const int32_t* row_items;
};

template <int VW, typename Fn>
__device__ __forceinline__ void for_row_items(RowItems ri, int64_t row, int lane, Fn&& fn) {
  const int64_t j0 = ri.row_ptr[row], j1 = ri.row_ptr[row + 1];
  for (int64_t j = j0; j < j1; j += kWave) {
    const int n = static_cast<int>(min<int64_t>(kWave, j1 - j));
    const int ids = (lane < n) ? ri.row_items[j + lane] : 0;
    int t = 0;
    for (; t + 4 <= n; t += 4) {
      const int64_t i0 = __builtin_amdgcn_readlane(ids, t), i1 = __builtin_amdgcn_readlane(ids, t + 1);
      const int64_t i2 = __builtin_amdgcn_readlane(ids, t + 2), i3 = __builtin_amdgcn_readlane(ids, t + 3);
      fn(i0, i1, i2, i3, 4);
    }
    for (; t < n; ++t) {
      const int64_t i0 = __builtin_amdgcn_readlane(ids, t);
      fn(i0, i0, i0, i0, 1);
    }
  }
}

// The ordered reduce's body: the lane's VW columns of the row's slab rows folded in item order.
// k_seg_reduce (FoldSum) and k_seg_reduce_red (FoldMax) differ in the fold and in what they write.
template <int VW, class Fold>
__device__ __forceinline__ void seg_reduce_fold(const float* slabs, RowItems ri, int64_t row, int lane,
                                                Fold fold, float (&acc)[VW]) {
  const int col = lane * VW;
  constexpr int F = kWave * VW;
#pragma unroll
  for (int q = 0; q < VW; ++q) acc[q] = Fold::kInit;
  for_row_items<VW>(ri, row, lane, [&](int64_t i0, int64_t i1, int64_t i2, int64_t i3, int m) {
    Vec<VW> p[4];
    p[0].load(slabs + i0 * F + col);
    if (m == 4) {
      p[1].load(slabs + i1 * F + col);
      p[2].load(slabs + i2 * F + col);
      p[3].load(slabs + i3 * F + col);
    }
    for (int u = 0; u < m; ++u)
#pragma unroll
      for (int q = 0; q < VW; ++q) acc[q] = fold.combine(acc[q], p[u].v[q]);
  });
}

template <int VW>
__global__ void __launch_bounds__(kBlock)
k_seg_reduce(int64_t n_rows, const float* __restrict__ slabs, const float* __restrict__ row_scale,
             float* __restrict__ y, int64_t ldy, int accumulate, RowItems ri) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int col = lane * VW;
  float acc[VW];
  seg_reduce_fold<VW>(slabs, ri, row, lane, FoldSum<false>{}, acc);
  const float scale = row_scale ? row_scale[row] : 1.f;
  float* yp = y + row * ldy + col;
  Vec<VW> o;
  if (accumulate) {
    o.load(yp);
#pragma unroll
    for (int q = 0; q < VW; ++q) o.v[q] += scale * acc[q];
  } else {
#pragma unroll
    for (int q = 0; q < VW; ++q) o.v[q] = scale * acc[q];
  }
  o.store(yp);
}

// k_seg_reduce for gta_reduce_blocked: the row's slab rows (partial maxima in the MAX domain,
// k_red_seg4 / k_red_h32) folded with red_max and flipped back.  A row without items -- a row
// without edges -- gets 0, decided from its item count, never from the identity.
template <int VW>
__global__ void __launch_bounds__(kBlock)
k_seg_reduce_red(int64_t n_rows, const float* __restrict__ slabs, uint32_t sbit, float* __restrict__ y, int64_t ldy,
                 RowItems ri) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int col = lane * VW;
  const bool empty = ri.row_ptr[row] == ri.row_ptr[row + 1];
  float acc[VW];
  seg_reduce_fold<VW>(slabs, ri, row, lane, FoldMax<false>{0u}, acc);  // partials are in the MAX domain: no flip
  Vec<VW> o;
#pragma unroll
  for (int q = 0; q < VW; ++q) o.v[q] = empty ? 0.f : red_flip(acc[q], sbit);
  o.store(y + row * ldy + col);
}

// Ordered reduce of the attention form: y[row, c] = sf_out(sum_k acc_k / sum_k s_k[head(c)])
// (normalize; rows without edges get sf_out(0)), or of the numerator alone; sums[row, h] =
// sum_k s_k[h] when requested.  Slab rows hold F partials then H sums (stride F + H rounded up to 4);
// same item order as k_seg_reduce.  sf_out: an SF applied to y (GTA_SF_NONE: none) -- the SF that
// follows GAT's aggregate (op 13), fused so y is written once instead of twice.
template <int VW>
__global__ void __launch_bounds__(kBlock)
k_seg_reduce_att(int64_t n_rows, const float* __restrict__ slabs, int H, int normalize, float* __restrict__ y,
                 int64_t ldy, float* __restrict__ sums, RowItems ri, int skip_single = 0, int sf_out = GTA_SF_NONE) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  if (skip_single && ri.row_ptr[row + 1] - ri.row_ptr[row] == 1) return;  // written by its item
  const int col = lane * VW;
  constexpr int F = kWave * VW;
  const int64_t lds = F + ((H + 3) & ~3);
  const int head = col / (F / H);
  float acc[VW];
#pragma unroll
  for (int q = 0; q < VW; ++q) acc[q] = 0.f;
  float sh = 0.f, sl = 0.f;  // this lane's head sum; lane < H: head `lane`'s sum (for `sums`)
  const bool any = ri.row_ptr[row + 1] > ri.row_ptr[row];
  for_row_items<VW>(ri, row, lane, [&](int64_t i0, int64_t i1, int64_t i2, int64_t i3, int m) {
    const int64_t id[4] = {i0, i1, i2, i3};
    for (int u = 0; u < m; ++u) {
      Vec<VW> p;
      p.load(slabs + id[u] * lds + col);
#pragma unroll
      for (int q = 0; q < VW; ++q) acc[q] += p.v[q];
      const float* ss = slabs + id[u] * lds + F;
      sh += ss[head];
      if (lane < H) sl += ss[lane];
    }
  });
  Vec<VW> o;
#pragma unroll
  for (int q = 0; q < VW; ++q) o.v[q] = normalize ? (any ? acc[q] / sh : 0.f) : acc[q];
  if (sf_out != GTA_SF_NONE) {
#pragma unroll
    for (int q = 0; q < VW; ++q) o.v[q] = sf_apply(sf_out, o.v[q]);
  }
  o.store(y + row * ldy + col);
  if (sums != nullptr && lane < H) sums[row * H + lane] = sl;
}

// ---- column-blocked plan: segment table, heavy-first row order, bounded items ----
// A (block, row) segment of len edges becomes ceil(len / item_edges) items of
// near-equal length (empty segments none), so no single item's gather chain
// outlasts the rest of the launch (a Reddit row holds up to ~2.4e4 edges).  Item k
// writes slab row k; row_items lists each row's items in (block, part) order, the
// fixed order of the ordered reduce.
// Light rows merge blocks (row_edges > 0): a row of deg edges uses blocks of
// m = pow2 >= row_edges * B / deg fine blocks (m <= B), so its items still average
// ~row_edges edges instead of deg / B -- each item costs a start-up and a 512-B
// partial written and re-read, whatever its length.
// Item order (knob seg_class_major, default 1): the rows of one merge factor m = 2^c are a
// degree class c; the classes run one after the other, m = 1 (the heaviest rows) first, and a
// class's items are numbered merged-block-major over its own ceil(B / m) merged blocks, so
// the waves in flight gather from one slice of that class's width.  With 0 -- the order of
// every plan before the classes -- all rows are one class numbered fine-block-major, a merged
// block at its first fine block's position.  Partial grouping and each row's list are the
// same either way: the item order changes no bit of any result.
// layout (host-computable offsets first, then the item arrays):
//   int64 hdr[16] {B, bsize, n_rows, unsorted_flag, n_items, item_edges, max_items, row_items byte offset,
//                  row_edges, class_major}
//   int32 perm[n_rows]             rows, class-major, heaviest degree bucket first inside a class
//   int32 seg[n_rows*(B+1)]        per-row segment offsets
//   int32 bucket[2*256]            (count, offset) per (class, degree bucket) key
//   int32 cls[256]                 class table (kCls* offsets) and the first item id of every group
//   int64 row_ptr[n_rows+1]        exclusive scan of items per row
//   int32 cnt[n_rows*B]            items per (class, merged block, position in the class), scanned in
//                                  place to item offsets; sum_c ceil(B / m_c) * n_c <= n_rows * B used
//   SegItem items[max_items]       class-major, block-major inside a class, longest first inside a block
//   int32 row_items[max_items]     item ids of each row, (block, part) order
constexpr int kMaxCls = 7;       // m = 1, 2, ..., 64 (B <= 63)
constexpr int kMaxGroups = 128;  // (class, merged block) groups: sum_c ceil(63 / 2^c) = 126
constexpr int kClsBase = 0;      // [kMaxCls + 1] first cnt entry of the class (the last: entries in use)
constexpr int kClsRow0 = 8;      // [kMaxCls] first perm position
constexpr int kClsRows = 16;     // [kMaxCls] rows
constexpr int kClsStep = 24;     // [kMaxCls] fine blocks per group (m; 1 when not class-major)
constexpr int kClsGroup0 = 32;   // [kMaxCls + 1] first group (the last: groups in all)
constexpr int kClsFirst = 48;    // [kMaxGroups + 1] first item id of group g (the last: n_items)

struct BlockedView {
  int64_t* hdr;
  int32_t* perm;
  int32_t* seg;
  int32_t* bucket;
  int32_t* cls;
  int64_t* row_ptr;
  int32_t* cnt;
  int64_t* scan;  // scan scratch (kScanMaxTiles + 1)
  int32_t* lhist;  // [2][kMaxGroups][kLenBins]: item-length histogram per group, then placement cursors
  SegItem* items;
  int32_t* row_items;
  int32_t* item_slot;  // position of item k in row_items (for the length sort)
  SegItem* items_tmp;  // length-sorted items before they are copied back
};

inline int64_t blocked_max_items(int64_t n_rows, int64_t nnz, int B, int64_t item_edges) {
  return std::min<int64_t>(n_rows * B, nnz) + nnz / item_edges;
}

constexpr int64_t kScanMaxTiles = 4096;  // plan-build scan (scan_excl): tile sums kept in the plan

constexpr int kLenBins = 257;  // item length keys 256 - min(len, 256): longest first

inline int64_t blocked_fixed_bytes(int64_t n_rows, int B) {
  return round16(128) + round16(n_rows * 4) + round16(n_rows * (B + 1) * 4) + round16(2 * 256 * 4) + round16(256 * 4) +
         round16((n_rows + 1) * 8) + round16(n_rows * B * 4) + round16((kScanMaxTiles + 1) * 8) +
         round16(2 * kMaxGroups * kLenBins * 4);
}

BlockedView blocked_view(void* base, int64_t n_rows, int B, int64_t max_items) {
  char* p = static_cast<char*>(base);
  BlockedView v;
  v.hdr = reinterpret_cast<int64_t*>(p); p += round16(16 * 8);
  v.perm = reinterpret_cast<int32_t*>(p); p += round16(n_rows * 4);
  v.seg = reinterpret_cast<int32_t*>(p); p += round16(n_rows * (B + 1) * 4);
  v.bucket = reinterpret_cast<int32_t*>(p); p += round16(2 * 256 * 4);
  v.cls = reinterpret_cast<int32_t*>(p); p += round16(256 * 4);
  v.row_ptr = reinterpret_cast<int64_t*>(p); p += round16((n_rows + 1) * 8);
  v.cnt = reinterpret_cast<int32_t*>(p); p += round16(n_rows * B * 4);
  v.scan = reinterpret_cast<int64_t*>(p); p += round16((kScanMaxTiles + 1) * 8);
  v.lhist = reinterpret_cast<int32_t*>(p); p += round16(2 * kMaxGroups * kLenBins * 4);
  v.items = reinterpret_cast<SegItem*>(p); p += round16(max_items * 16);
  v.row_items = reinterpret_cast<int32_t*>(p); p += round16(max_items * 4);
  v.item_slot = reinterpret_cast<int32_t*>(p); p += round16(max_items * 4);
  v.items_tmp = reinterpret_cast<SegItem*>(p);
  return v;
}

int64_t blocked_bytes(int64_t n_rows, int B, int64_t max_items) {
  return blocked_fixed_bytes(n_rows, B) + round16(max_items * 16) + round16(max_items * 4) + round16(max_items * 4) +
         round16(max_items * 16);
}

__device__ __forceinline__ int deg_bucket(int64_t d) {  // 31 = heaviest ... 0 = empty/1
  return d <= 1 ? 0 : min(31, 63 - __clzll(static_cast<unsigned long long>(d)));
}

__host__ __device__ __forceinline__ int64_t n_parts(int64_t len, int64_t item_edges) {
  return (len + item_edges - 1) / item_edges;
}

// fine blocks per merged block of a row with deg edges (1 = no merging)
__device__ __forceinline__ int merge_of(int64_t deg, int B, int64_t row_edges) {
  if (row_edges <= 0 || deg <= 0) return 1;
  int m = 1;
  while (m < B && deg * m < row_edges * B) m <<= 1;
  return m;
}

// (class, degree bucket) key of a row: class log2(m) when class-major, else one class
__device__ __forceinline__ int row_key(int64_t deg, int m, int class_major) {
  return (class_major ? (31 - __clz(m)) * 32 : 0) + deg_bucket(deg);
}

// one wave per row: lane b (0..B) binary-searches the first edge with col >= b*bsize;
// all lanes also verify the row's columns are sorted (the segments need it).  Also
// writes the row's item count (sum over blocks of n_parts) into row_ptr[row].
__global__ void __launch_bounds__(kBlock)
k_blocked_seg(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int B,
              int64_t bsize, int64_t item_edges, int64_t row_edges, int class_major, BlockedView v) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int64_t rb = indptr[row], re = indptr[row + 1];
  int64_t pos = 0;  // lane b < B+1: offset of block b
  for (int b = lane; b <= B; b += kWave) {
    const int64_t key = static_cast<int64_t>(b) * bsize;
    int64_t lo = rb, hi = re;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (static_cast<int64_t>(indices[mid]) < key) lo = mid + 1; else hi = mid;
    }
    pos = (b == B ? re : lo) - rb;
    v.seg[row * (B + 1) + b] = static_cast<int32_t>(pos);
  }
  // B <= 63: lane b holds offset b; lane j's merged block is [pos_{j*m}, pos_{min((j+1)*m, B)})
  const int m = merge_of(re - rb, B, row_edges);
  const int nb = (B + m - 1) / m;
  const int64_t lo = __shfl(pos, min(lane * m, B));
  const int64_t hi = __shfl(pos, min((lane + 1) * m, B));
  int64_t parts = (lane < nb) ? n_parts(hi - lo, item_edges) : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) parts += __shfl_xor(parts, off);
  if (lane == 0) v.row_ptr[row] = parts;
  bool bad = false;
  for (int64_t e = rb + lane; e + 1 < re; e += kWave) bad |= indices[e] > indices[e + 1];
  if (__any(bad) && lane == 0) atomicOr(reinterpret_cast<unsigned long long*>(&v.hdr[3]), 1ull);
  if (lane == 0) atomicAdd(&v.bucket[row_key(re - rb, m, class_major)], 1);
}

// row offsets per (class, bucket) key -- class m = 1 first, inside a class the heaviest bucket
// first -- and the class table: rows, first perm position, first cnt entry and first group
__global__ void k_blocked_scan(BlockedView v, int B, int class_major) {
  if (threadIdx.x != 0) return;
  int run = 0, base = 0, group = 0;
  for (int c = 0; c < kMaxCls; ++c) {
    const int step = class_major ? 1 << c : 1, nb = (B + step - 1) / step, row0 = run;
    for (int k = 31; k >= 0; --k) {
      v.bucket[256 + c * 32 + k] = run;
      run += v.bucket[c * 32 + k];
    }
    v.cls[kClsBase + c] = base;
    v.cls[kClsRow0 + c] = row0;
    v.cls[kClsRows + c] = run - row0;
    v.cls[kClsStep + c] = step;
    v.cls[kClsGroup0 + c] = group;
    // a class without rows (every class but the first when not class-major) has no groups
    if (run > row0) {
      base += nb * (run - row0);
      group += nb;
    }
  }
  v.cls[kClsBase + kMaxCls] = base;
  v.cls[kClsGroup0 + kMaxCls] = group;
}

__global__ void k_blocked_perm(const int64_t* __restrict__ indptr, int64_t n_rows, int B, int64_t row_edges,
                               int class_major, BlockedView v) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t deg = indptr[r + 1] - indptr[r];
  const int k = row_key(deg, merge_of(deg, B, row_edges), class_major);
  const int pos = atomicAdd(&v.bucket[256 + k], 1);  // order inside a bucket is free: results don't depend on it
  v.perm[pos] = static_cast<int32_t>(r);
}

// cnt entry k -> its class c, group (merged block of the class) j and row; false past the
// entries in use.  b = first fine block of the group.
struct CntEntry {
  int c, j, b;
  int32_t row;
};

__device__ __forceinline__ bool cnt_entry(const BlockedView& v, int64_t k, CntEntry& e) {
  if (k >= v.cls[kClsBase + kMaxCls]) return false;
  int c = 0;
  while (c + 1 < kMaxCls && k >= v.cls[kClsBase + c + 1]) ++c;  // empty classes share the next one's base
  const int64_t off = k - v.cls[kClsBase + c], n = v.cls[kClsRows + c];
  e.c = c;
  e.j = static_cast<int>(off / n);
  e.b = e.j * v.cls[kClsStep + c];
  e.row = v.perm[v.cls[kClsRow0 + c] + (off - e.j * n)];
  return true;
}

// cnt[k] = items of (class, group, row): the parts of the row's merged block starting at fine
// block b, 0 if none starts there (not class-major: a group is one fine block of all rows)
__global__ void k_blocked_cnt(int64_t n_rows, int B, int64_t item_edges, int64_t row_edges, BlockedView v) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (k >= n_rows * B) return;
  CntEntry e;
  if (!cnt_entry(v, k, e)) {
    v.cnt[k] = 0;
    return;
  }
  const int b = e.b;
  const int32_t* sg = v.seg + static_cast<int64_t>(e.row) * (B + 1);
  const int m = merge_of(sg[B], B, row_edges);
  v.cnt[k] = (b % m) ? 0 : static_cast<int32_t>(n_parts(sg[min(b + m, B)] - sg[b], item_edges));
}

// single-workgroup in-place exclusive scan (plan build only); out[n] = total when
// TOTAL_AT_END, and *total = the sum when total != nullptr
template <typename T>
__global__ void __launch_bounds__(1024) k_scan_excl(T* __restrict__ a, int64_t n, int total_at_end,
                                                    int64_t* __restrict__ total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t per = (n + 1023) / 1024;
  const int64_t b = min<int64_t>(n, t * per), e = min<int64_t>(n, b + per);
  int64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const int64_t x = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int64_t run = (t == 0) ? 0 : part[t - 1];
  for (int64_t i = b; i < e; ++i) {
    const int64_t x = a[i];
    a[i] = static_cast<T>(run);
    run += x;
  }
  if (t == 1023) {
    if (total_at_end) a[n] = static_cast<T>(part[1023]);
    if (total) *total = part[1023];
  }
}

// Multi-workgroup form of k_scan_excl for the large plan arrays (n_rows * B counts): tile b =
// [b * tile, (b + 1) * tile) of 1024 threads x kScanPer elements.  k_scan_tiles sums each tile
// (coalesced), k_scan_excl scans the tile sums (sums[nt] = total), k_scan_apply rescans each tile
// from its offset.  Same result as k_scan_excl.
constexpr int kScanPer = 16;
constexpr int64_t kScanTile = 1024 * kScanPer;

template <typename T>
__global__ void __launch_bounds__(1024) k_scan_tiles(const T* __restrict__ a, int64_t n, int64_t tile,
                                                     int64_t* __restrict__ sums) {
  __shared__ int64_t red[16];
  const int t = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * tile, b1 = min<int64_t>(n, b0 + tile);
  int64_t s = 0;
  for (int64_t i = b0 + t; i < b1; i += 1024) s += a[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    int64_t tot = 0;
    for (int w = 0; w < 16; ++w) tot += red[w];
    sums[blockIdx.x] = tot;
  }
}

template <typename T>
__global__ void __launch_bounds__(1024) k_scan_apply(T* __restrict__ a, int64_t n, int64_t tile,
                                                     const int64_t* __restrict__ offs, int64_t nt, int total_at_end,
                                                     int64_t* __restrict__ total) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * tile, b1 = min<int64_t>(n, b0 + tile);
  const int64_t per = tile / 1024;
  const int64_t e0 = min<int64_t>(b1, b0 + t * per), e1 = min<int64_t>(b1, e0 + per);
  int64_t s = 0;
  for (int64_t i = e0; i < e1; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // Hillis-Steele inclusive scan
    const int64_t x = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  int64_t run = offs[blockIdx.x] + ((t == 0) ? 0 : part[t - 1]);
  for (int64_t i = e0; i < e1; ++i) {
    const int64_t x = a[i];
    a[i] = static_cast<T>(run);
    run += x;
  }
  if (blockIdx.x == nt - 1 && t == 0) {
    if (total_at_end) a[n] = static_cast<T>(offs[nt]);
    if (total) *total = offs[nt];
  }
}

// exclusive scan of a[0, n) in place (a[n] = total when total_at_end; *total when given);
// scratch holds kScanMaxTiles + 1 int64
template <typename T>
void scan_excl(T* a, int64_t n, int total_at_end, int64_t* total, int64_t* scratch, hipStream_t s) {
  int64_t tile = kScanTile;
  while ((n + tile - 1) / tile > kScanMaxTiles) tile *= 2;
  const int64_t nt = (n + tile - 1) / tile;
  if (nt <= 1) {
    k_scan_excl<T><<<1, 1024, 0, s>>>(a, n, total_at_end, total);
    return;
  }
  k_scan_tiles<T><<<dim3(static_cast<unsigned>(nt)), dim3(1024), 0, s>>>(a, n, tile, scratch);
  k_scan_excl<int64_t><<<1, 1024, 0, s>>>(scratch, nt, 1, nullptr);
  k_scan_apply<T><<<dim3(static_cast<unsigned>(nt)), dim3(1024), 0, s>>>(a, n, tile, scratch, nt, total_at_end, total);
}

// items of cnt entry k (class, group, row): near-equal parts of the segment, item ids
// cnt[k] .. cnt[k] + parts - 1; each is also listed under its row, after the row's
// items of blocks < b
__global__ void k_blocked_items(const int64_t* __restrict__ indptr, int64_t n_rows, int B, int64_t item_edges,
                                int64_t row_edges, BlockedView v) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  CntEntry e;
  if (k >= n_rows * B || !cnt_entry(v, k, e)) return;
  const int b = e.b, group = v.cls[kClsGroup0 + e.c] + e.j;
  const int32_t row = e.row;
  const int32_t* sg = v.seg + static_cast<int64_t>(row) * (B + 1);
  const int m = merge_of(sg[B], B, row_edges);
  if (b % m) return;
  const int64_t len = sg[min(b + m, B)] - sg[b];
  if (len == 0) return;
  int64_t before = 0;  // the row's items in merged blocks before b
  for (int q = 0; q < b; q += m) before += n_parts(sg[min(q + m, B)] - sg[q], item_edges);
  const int64_t parts = n_parts(len, item_edges), part = (len + parts - 1) / parts;
  const int64_t id0 = v.cnt[k], slot0 = v.row_ptr[row] + before, beg = indptr[row] + sg[b];
  for (int64_t j = 0; j < parts; ++j) {
    SegItem it;
    it.beg = beg + j * part;
    it.row = row;
    it.len = static_cast<int32_t>(max<int64_t>(0, min<int64_t>(part, len - j * part)));
    v.items[id0 + j] = it;
    v.row_items[slot0 + j] = static_cast<int32_t>(id0 + j);
    v.item_slot[id0 + j] = static_cast<int32_t>(slot0 + j);
    atomicAdd(&v.lhist[group * kLenBins + 256 - min(it.len, 256)], 1);
  }
}

// length sort of each group's items (longest first), so the two half-wave items of a wave
// hold about the same number of edges and finish together.  Only item ids move: each row's
// row_items keep their (block, part) order, so the reduce -- and every result -- is unchanged.
__device__ __forceinline__ int len_key(int len) { return 256 - min(len, 256); }

// one thread per (class, merged block) group: its first item id (the scanned cnt entry of the
// group's first row) and the placement cursor of each of its length keys
__global__ void __launch_bounds__(kMaxGroups) k_items_len_scan(BlockedView v) {
  const int g = threadIdx.x, groups = v.cls[kClsGroup0 + kMaxCls];
  if (g == groups) v.cls[kClsFirst + g] = static_cast<int32_t>(v.hdr[4]);
  if (g >= groups) return;
  int c = 0;
  while (c + 1 < kMaxCls && g >= v.cls[kClsGroup0 + c + 1]) ++c;
  const int64_t k = v.cls[kClsBase + c] + static_cast<int64_t>(g - v.cls[kClsGroup0 + c]) * v.cls[kClsRows + c];
  int run = v.cnt[k];
  v.cls[kClsFirst + g] = run;
  for (int key = 0; key < kLenBins; ++key) {
    const int n = v.lhist[g * kLenBins + key];
    v.lhist[kMaxGroups * kLenBins + g * kLenBins + key] = run;
    run += n;
  }
}

__global__ void k_items_permute(BlockedView v) {
  const int64_t id = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (id >= v.hdr[4]) return;
  int lo = 0, hi = v.cls[kClsGroup0 + kMaxCls] - 1;  // the group holding item id: last g with first id <= id
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (v.cls[kClsFirst + mid] <= id) lo = mid; else hi = mid - 1;
  }
  const SegItem it = v.items[id];
  const int nid = atomicAdd(&v.lhist[kMaxGroups * kLenBins + lo * kLenBins + len_key(it.len)], 1);
  v.items_tmp[nid] = it;
  v.row_items[v.item_slot[id]] = nid;
}

// sum the chunk partials of split rows, in chunk order
__global__ void __launch_bounds__(kBlock)
k_aggregate_combine(PlanView plan, int F, const float* __restrict__ row_scale, float* __restrict__ y, int64_t ldy,
                    int accumulate, const float* __restrict__ partial, const void* __restrict__ xs = nullptr,
                    int64_t ldxs = 0, int xs_bf16 = 0, const float* __restrict__ self_scale = nullptr,
                    int y_bf16 = 0) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t s = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (s >= plan.hdr[1]) return;
  const int64_t row = plan.split_row[s];
  const int64_t first = plan.split_first[s];
  const int cnt = plan.split_cnt[s];
  const float scale = row_scale ? row_scale[row] : 1.f;
  for (int c = lane; c < F; c += kWave) {
    float a = 0.f;
    for (int j = 0; j < cnt; ++j) a += partial[(first + j) * F + c];
    float* yp = y + row * ldy + c;
    float v;
    if (xs != nullptr) {  // the self term, as k_aggregate forms it
#pragma clang fp contract(off)
      const float xv = xs_bf16 ? load_elem(static_cast<const uint16_t*>(xs) + row * ldxs + c)
                               : static_cast<const float*>(xs)[row * ldxs + c];
      v = xv * (self_scale ? *self_scale : 1.f) + scale * a;
    } else {
      v = accumulate ? (*yp + scale * a) : scale * a;
    }
    if (y_bf16) reinterpret_cast<uint16_t*>(y)[row * ldy + c] = to_bf16_bits(v);
    else *yp = v;
  }
}

// ---------------------------------------------------------------------------
// Shared pieces of the edge-wise / node-wise element kernels (K1, K3, K5) and
// of the unfused GAT softmax (K3', k_softmax_shift)
// ---------------------------------------------------------------------------
// A wave-per-row kernel's prologue: lane, row and the row's edge range; false past the last row
struct WaveRow {
  int lane;
  int64_t row, beg, end;
  __device__ __forceinline__ bool init(const int64_t* __restrict__ indptr, int64_t n_rows) {
    lane = threadIdx.x & (kWave - 1);
    row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
    if (row >= n_rows) return false;
    beg = indptr[row], end = indptr[row + 1];
    return true;
  }
};

// k_apply_edge_cols keeps its own text: edge_row is its row rule; ld_vec reads VW columns for it and for Operand
__device__ __forceinline__ int64_t edge_row(int mode, int64_t e, int64_t row, const int32_t* indices) {
  return mode == GTA_IDX_EDGE ? e : (mode == GTA_IDX_SRC ? static_cast<int64_t>(indices[e]) : row);
}
template <int VW>
__device__ __forceinline__ void ld_vec(const float* p, float* v, int ga, int c) {  // VW output columns from c
  if (ga == 1) {
    if (VW == 4) { const float4 t = *reinterpret_cast<const float4*>(p + c); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else if (VW == 2) { const float2 t = *reinterpret_cast<const float2*>(p + c); v[0] = t.x; v[1] = t.y; }
    else v[0] = p[c];
  } else {  // VW consecutive columns share one head (ga % VW == 0)
    const float t = p[c / ga];
#pragma unroll
    for (int q = 0; q < VW; ++q) v[q] = t;
  }
}


// One operand of an element kernel: p[rows, ld] read by edge (EDGE), by the edge's source (SRC) or
// by its destination row (DST); ld == 0 is one row for all (any row id times 0: the test below only
// keeps such an operand from reading source ids); output column c reads column c / g.
struct Operand {
  const float* p;
  int mode;
  int64_t ld;
  int g;
  // the row of edge e, whose destination is dst and whose source is src() (called in mode SRC only)
  template <class Src>
  __device__ __forceinline__ const float* row(int64_t e, int64_t dst, Src src) const {
    const int64_t r = mode == GTA_IDX_EDGE ? e : (mode == GTA_IDX_SRC ? (ld == 0 ? 0 : static_cast<int64_t>(src())) : dst);
    return p + r * ld;
  }
  __device__ __forceinline__ bool reads(int m) const { return p != nullptr && ld != 0 && mode == m; }  // row() uses m's ids
  __device__ __forceinline__ int col(int c) const { return c / g; }
};

// out = sf(bin(a, b)), or sf(a) without a b: the one combine of every K3 / K5 form
template <int VW>
__device__ __forceinline__ void combine(int bin, int sf, bool has_b, const Vec<VW>& va, const Vec<VW>& vb, Vec<VW>& out) {
#pragma unroll
  for (int q = 0; q < VW; ++q) out.v[q] = sf_apply(sf, has_b ? bin_apply(bin, va.v[q], vb.v[q]) : va.v[q]);
}

// The head-lane edge walk of a row (lane = k*H + h: edge slot k, head h): 64 indices per coalesced
// load, a full chunk in H steps with its gathers of b issued NB at a time, the last chunk masked;
// body(edge, b[src(edge), h]) once per edge and head, edges ascending per lane.  The full chunk
// shuffles with ds_bpermute itself (byte address 4 * slot), its base pinned inside the chunk loop:
// left loop-invariant every step's address gets a register of its own (79 VGPRs for 40 at H = 64).
template <int H, class Body>
__device__ __forceinline__ void head_lane_walk(int lane, int64_t beg, int64_t end, const int32_t* indices, const float* b,
                                               int64_t ldb, Body body) {
  constexpr int EPS = kWave / H;  // edges per step
  constexpr int NB = H < 8 ? H : 8;
  const int h = lane % H, k = lane / H;
  for (int64_t e0 = beg; e0 < end; e0 += kWave) {
    const int cnt = (end - e0 < kWave) ? static_cast<int>(end - e0) : kWave;
    const int mine = (lane < cnt) ? indices[e0 + lane] : 0;
    if (cnt == kWave) {  // H steps of EPS edges, gathers issued NB at a time
      int base = 4 * k;
      asm volatile("" : "+v"(base));  // the pin
#pragma unroll
      for (int j0 = 0; j0 < H; j0 += NB) {
        float v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const int src = __builtin_amdgcn_ds_bpermute(4 * (j0 + j) * EPS + base, mine);
          v[j] = b[static_cast<int64_t>(src) * ldb + h];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) body(e0 + (j0 + j) * EPS + k, v[j]);
      }
    } else {
      for (int j = 0; j * EPS < cnt; ++j) {
        const int slot = j * EPS + k;
        const int src = __shfl(mine, slot < cnt ? slot : 0);
        if (slot < cnt) body(e0 + slot, b[static_cast<int64_t>(src) * ldb + h]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// K1 scatter: byte-exact row copies node -> edge, one wave per destination row
// ---------------------------------------------------------------------------
template <typename UNIT>
__global__ void __launch_bounds__(kBlock)
k_scatter(int dir, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
          const UNIT* __restrict__ x, int64_t ldx_u, int64_t row_u, UNIT* __restrict__ out, int64_t ldo_u) {
  WaveRow w;
  if (!w.init(indptr, n_rows)) return;
  const int64_t total = (w.end - w.beg) * row_u;
  for (int64_t t = w.lane; t < total; t += kWave) {
    const int64_t el = t / row_u, c = t - el * row_u;
    const int64_t e = w.beg + el;
    const int64_t src = (dir == GTA_DIR_R) ? w.row : indices[e];
    out[e * ldo_u + c] = x[src * ldx_u + c];
  }
}

// ---------------------------------------------------------------------------
// K3 apply_edge / K5 apply_node: element-wise with head broadcast + SF
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_apply_edge(int bin, int sf, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
             int64_t n_rows, const float* __restrict__ a, int a_mode, int64_t lda, int Fa,
             const float* __restrict__ b, int b_mode, int64_t ldb, int Fb, float* __restrict__ out,
             int64_t ldo, int Fo) {
  WaveRow w;
  if (!w.init(indptr, n_rows)) return;
  const int64_t total = (w.end - w.beg) * Fo;
  const Operand A{a, a_mode, lda, Fo / Fa}, B{b, b_mode, ldb, (b != nullptr) ? Fo / Fb : 1};
  for (int64_t t = w.lane; t < total; t += kWave) {
    const int64_t el = t / Fo;
    const int c = static_cast<int>(t - el * Fo);
    const int64_t e = w.beg + el;
    const auto src = [&] { return indices[e]; };
    Vec<1> va, vb;
    va.v[0] = A.row(e, w.row, src)[A.col(c)];
    if (b != nullptr) vb.v[0] = B.row(e, w.row, src)[B.col(c)];
    combine<1>(bin, sf, b != nullptr, va, vb, va);
    out[e * ldo + c] = va.v[0];
  }
}

// Row-sweep forms of K3 (the generic kernel above divides per element and re-reads
// the index per element).  A wave owns a destination row and walks its edges:
//  * k_apply_edge_cols: lanes cover the output columns, VW per lane (float4/float2
//    when rows are aligned and any head broadcast keeps VW columns in one head),
//    4 edges unrolled so their row gathers are in flight together;
//  * k_apply_edge_pack: Fo <= 32 (a power of two): 64/Fo edges per wave instruction,
//    lane = (edge slot, column).
template <int VW>
__global__ void __launch_bounds__(kBlock)
k_apply_edge_cols(int bin, int sf, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                  int64_t n_rows, const float* __restrict__ a, int a_mode, int64_t lda, int ga,
                  const float* __restrict__ b, int b_mode, int64_t ldb, int gb, float* __restrict__ out,
                  int64_t ldo, int Fo) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int64_t eb = indptr[row], ee = indptr[row + 1];
  for (int c = lane * VW; c < Fo; c += kWave * VW) {
    int64_t e = eb;
    for (; e + 4 <= ee; e += 4) {
      float va[4][VW], vb[4][VW];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t ra = edge_row(a_mode, e + u, row, indices);
        ld_vec<VW>(a + ra * lda, va[u], ga, c);
        if (b != nullptr) {
          const int64_t rb = (ldb == 0) ? 0 : edge_row(b_mode, e + u, row, indices);
          ld_vec<VW>(b + rb * ldb, vb[u], gb, c);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float o[VW];
#pragma unroll
        for (int q = 0; q < VW; ++q) o[q] = sf_apply(sf, b != nullptr ? bin_apply(bin, va[u][q], vb[u][q]) : va[u][q]);
        float* op = out + (e + u) * ldo + c;
        if (VW == 4) *reinterpret_cast<float4*>(op) = make_float4(o[0], o[1], o[2], o[3]);
        else if (VW == 2) *reinterpret_cast<float2*>(op) = make_float2(o[0], o[1]);
        else op[0] = o[0];
      }
    }
    for (; e < ee; ++e) {
      float va[VW], vb[VW];
      ld_vec<VW>(a + edge_row(a_mode, e, row, indices) * lda, va, ga, c);
      if (b != nullptr) ld_vec<VW>(b + ((ldb == 0) ? 0 : edge_row(b_mode, e, row, indices)) * ldb, vb, gb, c);
      float* op = out + e * ldo + c;
#pragma unroll
      for (int q = 0; q < VW; ++q) op[q] = sf_apply(sf, b != nullptr ? bin_apply(bin, va[q], vb[q]) : va[q]);
    }
  }
}

// Round 6: the edge-parallel form (gta_apply_edge_flat) for outputs of exactly 64 * VW columns:
// a wave takes 32 consecutive edges whatever their rows -- so Flickr's 10-edge rows no longer leave
// a wave a few edges and three dependent round trips (row bounds, indices, rows) each -- reads their
// source ids and destination rows (the graph's cached edge -> row table) in one coalesced load,
// and walks them 8 at a time: each edge's operand rows are uniform addresses (readlane), one
// 64-lane instruction per 512-B row, 8 edges' rows in flight.  Per element the same
// sf(bin(a, b)) as every K3 form: bitwise equal to them.
template <int VW>
__global__ void __launch_bounds__(kBlock)
k_apply_edge_flat(int bin, int sf, const int32_t* __restrict__ erow, const int32_t* __restrict__ indices, int64_t nnz,
                  const float* __restrict__ a, int a_mode, int64_t lda, int ga, const float* __restrict__ b, int b_mode,
                  int64_t ldb, int gb, float* __restrict__ out, int64_t ldo) {
  constexpr int EPW = 32, U = 8;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t e0 = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform()) * EPW;
  if (e0 >= nnz) return;
  const int n = static_cast<int>(min<int64_t>(EPW, nnz - e0));
  const Operand A{a, a_mode, lda, ga}, B{b, b_mode, ldb, gb};
  const int src = ((A.reads(GTA_IDX_SRC) || B.reads(GTA_IDX_SRC)) && lane < n) ? indices[e0 + lane] : 0;
  const int dst = ((A.reads(GTA_IDX_DST) || B.reads(GTA_IDX_DST)) && lane < n) ? erow[e0 + lane] : 0;
  const int c = lane * VW;
  for (int u0 = 0; u0 < n; u0 += U) {
    Vec<VW> va[U], vb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u0 + u < n) {  // u0 + u: uniform edge slot of this chunk, so every row id is a uniform value
        const int64_t d = __builtin_amdgcn_readlane(dst, u0 + u);
        const auto s = [&] { return __builtin_amdgcn_readlane(src, u0 + u); };
        ld_vec<VW>(A.row(e0 + u0 + u, d, s), va[u].v, A.g, c);
        if (b != nullptr) ld_vec<VW>(B.row(e0 + u0 + u, d, s), vb[u].v, B.g, c);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u0 + u < n) {
        Vec<VW> o;
        combine<VW>(bin, sf, b != nullptr, va[u], vb[u], o);
        o.store(out + (e0 + u0 + u) * ldo + c);
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock)
k_apply_edge_pack(int bin, int sf, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                  int64_t n_rows, const float* __restrict__ a, int a_mode, int64_t lda, int ga,
                  const float* __restrict__ b, int b_mode, int64_t ldb, int gb, float* __restrict__ out,
                  int64_t ldo, int Fo) {
  WaveRow w;
  if (!w.init(indptr, n_rows)) return;
  const Operand A{a, a_mode, lda, ga}, B{b, b_mode, ldb, gb};
  const int epi = kWave / Fo, k = w.lane / Fo, c = w.lane - k * Fo;
  const int ca = A.col(c), cb = B.col(c);
  for (int64_t e0 = w.beg; e0 < w.end; e0 += epi) {
    const int64_t e = e0 + k;
    if (e < w.end) {
      const auto src = [&] { return indices[e]; };
      Vec<1> va, vb;
      va.v[0] = A.row(e, w.row, src)[ca];
      if (b != nullptr) vb.v[0] = B.row(e, w.row, src)[cb];
      combine<1>(bin, sf, b != nullptr, va, vb, va);
      out[e * ldo + c] = va.v[0];
    }
  }
}

template <typename TA>
__global__ void __launch_bounds__(kBlock)
k_apply_node(int bin, int sf, int64_t n, const TA* __restrict__ a, int64_t lda, int Fa,
             const float* __restrict__ b, int64_t ldb, int Fb, float* __restrict__ out, int64_t ldo, int Fo) {
  const int64_t total = n * Fo;
  const int ga = Fo / Fa, gb = (b != nullptr) ? Fo / Fb : 1;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = t / Fo;
    const int c = static_cast<int>(t - i * Fo);
    float va = load_elem(a + i * lda + c / ga);
    if (b != nullptr) va = bin_apply(bin, va, b[i * ldb + c / gb]);
    out[i * ldo + c] = sf_apply(sf, va);
  }
}

// Vector form of k_apply_node for the common shapes (same per-element ops, so bitwise equal):
// a and out [n, F] with F % 4 == 0 and 16-B rows, b none (BM 0), [n, F] (BM 1) or one value
// per node b[i * ldb] (BM 2; ldb 0 = one value for all, e.g. GIN's 1 + eps).  One float4 per
// thread step, 32-bit index math (n * F / 4 < 2^32).
template <int BM, typename TA = float>
__global__ void __launch_bounds__(kBlock)
k_apply_node4(int bin, int sf, uint32_t n4, uint32_t F4, const TA* __restrict__ a, int64_t lda,
              const float* __restrict__ b, int64_t ldb, float* __restrict__ out, int64_t ldo) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += gridDim.x * blockDim.x) {
    const uint32_t i = t / F4, c = (t - i * F4) * 4u;
    Vec<4> va, vb;
    load_row(va, a + i * lda + c);
    if (BM == 1) {
      vb.load(b + i * ldb + c);
    } else if (BM == 2) {
      const float t = b[i * ldb];
#pragma unroll
      for (int q = 0; q < 4; ++q) vb.v[q] = t;
    }
    combine<4>(bin, sf, BM != 0, va, vb, va);
    va.store(out + i * ldo + c);
  }
}

// ---------------------------------------------------------------------------
// K3' fused GAT edge-softmax: one wave per destination row; lane = k*H + h
// handles edge slot k (64/H edges per step) and head h.  Indices arrive 64 at
// a time (one coalesced load) and are handed to the lanes with ds_bpermute;
// each step gathers H consecutive floats of b_src per edge.  Pass 1 sums v per
// lane, a butterfly over the k bits gives the row sum per head; pass 2
// recomputes v (same bits) and writes v / sum -- one contiguous 256-B store per
// step.  normalize = 0 writes v in pass 1 and skips pass 2.
// ---------------------------------------------------------------------------
// SH: the shifted weight, v = expf(g(a + b) - shift[row, h]) (sf an exp-form, checked by the host).
template <int H, bool SH = false>
__global__ void __launch_bounds__(kBlock)
k_edge_softmax(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
               const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int sf,
               int normalize, float* __restrict__ out, float* __restrict__ sums,
               const float* __restrict__ shift = nullptr) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int h = lane % H, k = lane / H;
  const int64_t beg = indptr[row], end = indptr[row + 1];
  const float ar = a[row * lda + h];
  const float mr = SH ? shift[row * H + h] : 0.f;
  float s = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    const float inv = s;  // pass 1: row sum (division below, not a reciprocal)
    head_lane_walk<H>(lane, beg, end, indices, b, ldb, [&](int64_t e, float bv) __attribute__((always_inline)) {
      const float x = SH ? sf_shift(sf, ar + bv, mr) : sf_apply(sf, ar + bv);
      float* o = out + e * H + h;
      if (pass == 0) {
        s += x;
        if (!normalize) *o = x;
      } else {
        *o = x / inv;
      }
    });
    if (pass == 0) {
#pragma unroll
      for (int off = H; off < kWave; off <<= 1) s += __shfl_xor(s, off);
      if (sums != nullptr && k == 0) sums[row * H + h] = s;
      if (!normalize) break;
    }
  }
}

// Edge-per-lane form for H in {4, 8, 16} (16-B aligned rows): lane l owns edge
// e0 + l of a 64-edge chunk and loads its H source scores as H/4 float4 -- one
// gather per edge per row visit.  The first K chunks of the row keep v in
// VGPRs; later chunks park v in `out` during pass 1 and pass 2 reads it back
// (coalesced), so every source row is gathered exactly once.  Row sums: per
// lane, then a butterfly over all 64 lanes.
template <int H, int K, bool SH = false>
__global__ void __launch_bounds__(kBlock)
k_edge_softmax_v(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
                 const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int sf,
                 int normalize, float* __restrict__ out, float* __restrict__ sums,
                 const float* __restrict__ shift = nullptr) {
  constexpr int Q = H / 4;
  WaveRow w;
  if (!w.init(indptr, n_rows)) return;
  const int lane = w.lane;
  const int64_t row = w.row, beg = w.beg, end = w.end;
  float ar[H], s[H], mr[SH ? H : 1];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    ar[h] = a[row * lda + h];
    s[h] = 0.f;
    if (SH) mr[h] = shift[row * H + h];
  }
  float4 keep[K][Q];
  auto visit = [&](int64_t e0, float4 (&v)[Q]) {  // gather + sf for the chunk at e0; returns v in place
    const int64_t e = e0 + lane;
    const bool ok = e < end;
    const int src = ok ? indices[e] : 0;
    const float4* bp = reinterpret_cast<const float4*>(b + static_cast<int64_t>(src) * ldb);
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = ok ? bp[q] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float* c = reinterpret_cast<float*>(&v[q]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float sv = ar[4 * q + t] + c[t];
        const float x = ok ? (SH ? sf_shift(sf, sv, mr[SH ? 4 * q + t : 0]) : sf_apply(sf, sv)) : 0.f;
        c[t] = x;
        s[4 * q + t] += x;
      }
    }
    return ok;
  };
  const auto chunk = [&](int64_t e0) { return reinterpret_cast<float4*>(out + (e0 + lane) * H); };  // this lane's edge
  const auto put = [&](int64_t e0, const float4 (&v)[Q]) {
    float4* o = chunk(e0);
#pragma unroll
    for (int q = 0; q < Q; ++q) o[q] = v[q];
  };
  const auto div4 = [&](float4 v, int q) {  // v / s for heads 4q .. 4q + 3
    return make_float4(v.x / s[4 * q], v.y / s[4 * q + 1], v.z / s[4 * q + 2], v.w / s[4 * q + 3]);
  };
  // pass 1
  int64_t e0 = beg;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    if (e0 < end) {
      const bool ok = visit(e0, keep[c]);
      if (!normalize && ok) put(e0, keep[c]);
    }
    e0 += kWave;
  }
  for (int64_t f0 = beg + K * kWave; f0 < end; f0 += kWave) {
    float4 v[Q];
    if (visit(f0, v)) put(f0, v);
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) s[h] += __shfl_xor(s[h], off);
  }
  if (sums != nullptr && lane < H) {
    float sv = s[0];
#pragma unroll
    for (int h = 1; h < H; ++h) sv = (lane == h) ? s[h] : sv;
    sums[row * H + lane] = sv;
  }
  if (!normalize) return;
  // pass 2: v / s
  e0 = beg;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    if (e0 + lane < end) {
#pragma unroll
      for (int q = 0; q < Q; ++q) keep[c][q] = div4(keep[c][q], q);
      put(e0, keep[c]);
    }
    e0 += kWave;
  }
  for (int64_t f0 = beg + K * kWave; f0 < end; f0 += kWave) {
    if (f0 + lane < end) {
      float4* o = chunk(f0);
#pragma unroll
      for (int q = 0; q < Q; ++q) o[q] = div4(o[q], q);
    }
  }
}

// The shifted softmax's row maxima: shift[row, h] = max over the row's edges of g(a[row, h] +
// b[src, h]) for sf = exp . g.  fp32 addition and g are monotone non-decreasing in b, so this is
// g(a[row, h] + max_e b[src(e), h]) bit for bit: a max over b alone, g applied once.  One wave
// per row, lane = k*H + h as in k_edge_softmax: 64 indices per coalesced load, H consecutive
// floats of b per edge, gathers issued NB at a time.  red_max propagates NaN (a poisoned guard
// band must not be swallowed); idle slots hold -inf; a row without edges gets 0, decided from
// its degree.
template <int H>
__global__ void __launch_bounds__(kBlock)
k_softmax_shift(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
                const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, int sf,
                float* __restrict__ shift) {
  WaveRow w;
  if (!w.init(indptr, n_rows)) return;
  const int h = w.lane % H, k = w.lane / H;
  float m = -INFINITY;
  head_lane_walk<H>(w.lane, w.beg, w.end, indices, b, ldb,
                    [&](int64_t, float bv) __attribute__((always_inline)) { m = red_max(m, bv); });
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) m = red_max(m, __shfl_xor(m, off));
  if (k == 0) shift[w.row * H + h] = (w.end > w.beg) ? sf_g(sf, a[w.row * lda + h] + m) : 0.f;
}

// ---------------------------------------------------------------------------
// K4 UPDATE: out = sf(X[r(m)] . W), fp32 via v_mfma_f32_16x16x4_f32.
// Block tile 64x64, BK = 16, 4 waves as 2x2, each wave 32x32 = 2x2 MFMA tiles.
// MFMA 16x16x4 f32 maps (cdna_hip_programming.md §3): lane l holds
//   A[i = l&15][k = l>>4], B[k = l>>4][j = l&15]; D col = l&15, row = 4*(l>>4)+r.
// ---------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

// SF epilogue of the MFMA GEMMs applied to the whole accumulator tile in place, the switch on sf
// OUTSIDE the element loops.  With sf_apply per element each of the FR x NT x 4 store sites held
// its own switch over every SF body: the 8-deep k_mm_ring<8, 8, 2> of that time (since removed)
// compiled to 147 KB, and an epilogue run
// walked ~100 KB of cold instruction cache (each new lane of code an L2 round trip), a fixed
// ~10 us per launch that a 9-stage split-K block could not hide.  Here the no-SF path is one branch.
template <int FR, int NT>
__device__ __forceinline__ void sf_tile(int sf, f32x4 (&acc)[FR][NT]) {
  switch (sf) {
#define GTA_SFT(K_)                                                                  \
  case K_:                                                                           \
    _Pragma("unroll") for (int i = 0; i < FR; ++i)                                    \
      _Pragma("unroll") for (int c = 0; c < NT; ++c)                                  \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) acc[i][c][r] = sf_apply(K_, acc[i][c][r]); \
    return;
    GTA_SFT(GTA_SF_RELU) GTA_SFT(GTA_SF_EXP_LEAKY_RELU) GTA_SFT(GTA_SF_ELU) GTA_SFT(GTA_SF_EXP)
    GTA_SFT(GTA_SF_LEAKY_RELU) GTA_SFT(GTA_SF_SIGMOID) GTA_SFT(GTA_SF_TANH) GTA_SFT(GTA_SF_RECIP)
#undef GTA_SFT
    default: return;  // GTA_SF_NONE
  }
}

__global__ void __launch_bounds__(kBlock)
k_mm_f32(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ row_idx, int64_t M, int K,
         const float* __restrict__ w, int64_t ldw, int N, int sf, float* __restrict__ out, int64_t ldo) {
  constexpr int BM = 64, BN = 64, BK = 16;
  __shared__ float As[BM][BK + 1];
  __shared__ float Bs[BK][BN + 4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A loader: row = t/4, k = (t%4)*4 .. +3 ; B loader: k = t/16, n = (t%16)*4 .. +3
  const int ar = t >> 2, ak = (t & 3) * 4;
  const int64_t am = m0 + ar;
  const bool arow_ok = am < M;
  const int64_t asrc = arow_ok ? (row_idx ? static_cast<int64_t>(row_idx[am]) : am) : 0;
  const float* ap = x + asrc * ldx;
  const int bk = t >> 4, bn = (t & 15) * 4;

  for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + ak + q;
      As[ar][ak + q] = (arow_ok && k < K) ? ap[k] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = k0 + bk, n = n0 + bn + q;
      Bs[bk][bn + q] = (k < K && n < N) ? w[static_cast<int64_t>(k) * ldw + n] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = As[wr * 32 + i * 16 + (lane & 15)][kk + (lane >> 4)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = Bs[kk + (lane >> 4)][wc * 32 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wr * 32 + i * 16 + (lane >> 4) * 4 + r;
        const int n = n0 + wc * 32 + j * 16 + (lane & 15);
        if (m < M && n < N) out[m * ldo + n] = sf_apply(sf, acc[i][j][r]);
      }
}

// bf16 UPDATE via v_mfma_f32_16x16x32_bf16 (fp32 accumulate).  Block 64x64,
// BK = 32.  Lane l holds A[row l&15][k = 8(l>>4)+j] and B[k = 8(l>>4)+j][col l&15],
// j = 0..7 (cdna_hip_programming.md §3); B is staged transposed in LDS so both
// fragments are one 16-B LDS read.
typedef short bf16x8 __attribute__((ext_vector_type(8)));


template <typename TA>
__global__ void __launch_bounds__(kBlock)
k_mm_bf16(const TA* __restrict__ x, int64_t ldx, const int32_t* __restrict__ row_idx, int64_t M, int K,
          const uint16_t* __restrict__ w, int64_t ldw, int N, int sf, float* __restrict__ out, int64_t ldo) {
  constexpr int BM = 64, BN = 64, BK = 32, PAD = 8;
  __shared__ __attribute__((aligned(16))) uint16_t As[BM][BK + PAD];
  __shared__ __attribute__((aligned(16))) uint16_t Bt[BN][BK + PAD];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wr = wv >> 1, wc = wv & 1;
  const int64_t m0 = static_cast<int64_t>(blockIdx.x) * BM;
  const int n0 = blockIdx.y * BN;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ar = t >> 2, ak = (t & 3) * 8;  // A: 64 rows x 32 k, 8 per thread
  const int64_t am = m0 + ar;
  const bool arow_ok = am < M;
  const int64_t asrc = arow_ok ? (row_idx ? static_cast<int64_t>(row_idx[am]) : am) : 0;
  const TA* ap = x + asrc * ldx;
  constexpr bool kBf16A = sizeof(TA) == 2;
  const bool avec = kBf16A && ((ldx & 7) == 0) && aligned(x, 16);
  const int bk = t >> 3, bn = (t & 7) * 8;  // B: 32 k x 64 n, 8 per thread

  for (int k0 = 0; k0 < K; k0 += BK) {
    if (avec && arow_ok && k0 + ak + 8 <= K) {
      *reinterpret_cast<uint4*>(&As[ar][ak]) = *reinterpret_cast<const uint4*>(ap + k0 + ak);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = k0 + ak + q;
        As[ar][ak + q] = (arow_ok && k < K) ? to_bf16_bits(ap[k]) : static_cast<uint16_t>(0);
      }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int k = k0 + bk, n = n0 + bn + q;
      Bt[bn + q][bk] = (k < K && n < N) ? w[static_cast<int64_t>(k) * ldw + n] : static_cast<uint16_t>(0);
    }
    __syncthreads();
    bf16x8 af[2], bfr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
      af[i] = *reinterpret_cast<const bf16x8*>(&As[wr * 32 + i * 16 + (lane & 15)][8 * (lane >> 4)]);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      bfr[j] = *reinterpret_cast<const bf16x8*>(&Bt[wc * 32 + j * 16 + (lane & 15)][8 * (lane >> 4)]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t m = m0 + wr * 32 + i * 16 + (lane >> 4) * 4 + r;
        const int n = n0 + wc * 32 + j * 16 + (lane & 15);
        if (m < M && n < N) out[m * ldo + n] = sf_apply(sf, acc[i][j][r]);
      }
}

// ---- pieces shared by the MFMA UPDATE kernels (k_mm_rows, k_mm_ring, k_mm_wave, k_mm_ring_bf, k_mlp_bf) ----
// An MFMA 16x16 tile leaves lane (g, r16 = 4q + p) with C[4g + r][4q + p], r = 0..3.  A 4x4
// transpose inside each lane quad (DPP swaps of lane bit 0, then bit 1) turns that into
// C[4g + p][4q + r]: four consecutive columns of one row, one 16-B store instead of four dwords.
__device__ __forceinline__ void quad_transpose(float (&v)[4], int p) {
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2) {  // bit 0: registers (2m2, 2m2+1) across lanes (p, p^1)
    const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2]), 0xB1, 0xF, 0xF, false));
    const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2 + 1]), 0xB1, 0xF, 0xF, false));
    if (p & 1) v[2 * m2] = sb; else v[2 * m2 + 1] = sa;
  }
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2) {  // bit 1: registers (m2, m2+2) across lanes (p, p^2)
    const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2]), 0x4E, 0xF, 0xF, false));
    const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2 + 2]), 0x4E, 0xF, 0xF, false));
    if (p & 2) v[m2] = sb; else v[m2 + 2] = sa;
  }
}

// The accumulators of a (16 FR) x (16 NT) wave tile, rows from mw and columns from n0, out (the SF
// already applied: sf_tile): quad-transposed 16-B row stores when out rows are 16-B aligned
// (vstore), per element at a column tail and otherwise.  Rows past M and columns past N are skipped.
template <int FR, int NT>
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[FR][NT], float* __restrict__ out, int64_t ldo, int64_t M,
                                           int N, int64_t mw, int n0, int lane, bool vstore) {
  const int g = lane >> 4, r16 = lane & 15;
  if (vstore) {
    const int p = r16 & 3, q = r16 >> 2;
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = acc[i][c][r];
        quad_transpose(v, p);
        const int64_t m = mw + 16 * i + 4 * g + p;
        const int n = n0 + 16 * c + 4 * q;
        if (m < M) {
          if (n + 3 < N) {
            *reinterpret_cast<float4*>(out + m * ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (n + r < N) out[m * ldo + n + r] = v[r];
          }
        }
      }
  } else {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = mw + 16 * i + 4 * g + r;
          const int n = n0 + 16 * c + r16;
          if (m < M && n < N) out[m * ldo + n] = acc[i][c][r];
        }
  }
}

template <int FR, int NT>
__device__ __forceinline__ void zero_tile(f32x4 (&acc)[FR][NT]) {
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int c = 0; c < NT; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One 16-k fp32 step on fragments in registers: FR x NT x 4 v_mfma_f32_16x16x4_f32.  jj outermost:
// each of the FR x NT accumulators is touched once per FR * NT MFMAs; per accumulator the k order
// is k_mm_rows' (bitwise equal to it).
template <int FR, int NT>
__device__ __forceinline__ void mma_f32_step(f32x4 (&acc)[FR][NT], const f32x4 (&a4)[FR], const f32x4 (&b4)[NT]) {
#pragma unroll
  for (int jj = 0; jj < 4; ++jj)
#pragma unroll
    for (int c = 0; c < NT; ++c)
#pragma unroll
      for (int i = 0; i < FR; ++i)
        acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i][jj], b4[c][jj], acc[i][c], 0, 0, 0);
}

// Split K: block row y contracts k in [y * kslice, (y + 1) * kslice) into its own partial
// out + y * oslice; k_mm_slices_sum adds the slices in order.
template <typename PX, typename PW, typename PO>
__device__ __forceinline__ void split_k_slice(PX& x, PW& wt, PO& out, int& K, int64_t kslice, int64_t oslice) {
  const int64_t kb = static_cast<int64_t>(blockIdx.y) * kslice;
  x += kb;
  wt += kb;
  K = static_cast<int>(min<int64_t>(kslice, K - kb));
  out += static_cast<int64_t>(blockIdx.y) * oslice;
}

// Row-streaming UPDATE for the skinny shapes of GNN layers (M = nodes or edges,
// K and N at most a few hundred).  A block owns BN = 16*NT output columns (all of
// N up to 128, so X is read from HBM once) and walks 128-row groups g, g+grid, ...
// Each wave holds 32 rows x BN in MFMA accumulators; its A fragments come
// straight from global memory in the MFMA register layout (no LDS round trip).
// W arrives TRANSPOSED (wt[n][k]) and is staged per K chunk into LDS with 16-B
// copies -- once per block when K fits one chunk -- so a B fragment is one 16-B
// LDS read.
//   fp32:  v_mfma_f32_16x16x4_f32, lane (r, g) loads x[r][k0+4g .. +3]; sub-step j
//          contracts k = k0+4g+j (B read with the same k map).
//   bf16:  v_mfma_f32_16x16x32_bf16, lane (r, g) holds x[r][k0+8g .. +7] (fp32 X is
//          rounded to bf16 in registers, round to nearest even).
template <typename TA, typename WT, int NT, bool PF = false>  // PF: prefetch the next A fragment
__global__ void __launch_bounds__(kBlock, PF ? 4 : 1)
k_mm_rows(const TA* __restrict__ x, int64_t ldx, const int32_t* __restrict__ row_idx, int64_t M, int K,
          const WT* __restrict__ wt, int64_t ldwt, int N, int sf, float* __restrict__ out, int64_t ldo,
          int64_t kslice = 0, int64_t oslice = 0, int vec_store = 0) {
  if (kslice > 0) {  // split K: a partial sum takes no SF
    split_k_slice(x, wt, out, K, kslice, oslice);
    sf = GTA_SF_NONE;
  }
  constexpr bool BF = sizeof(WT) == 2;
  constexpr int KS = BF ? 32 : 16;         // k covered by one A-fragment load
  constexpr int KC = BF ? (NT >= 8 ? 128 : 256) : (NT >= 8 ? 64 : 128);  // K chunk staged in LDS (<= 35 KB)
  constexpr int KP = KC + (BF ? 8 : 4);    // padded LDS row (16-B aligned)
  constexpr int BN = 16 * NT;
  constexpr int WV = 16 / sizeof(WT);      // W elements per 16-B copy
  __shared__ __attribute__((aligned(16))) WT Bt[BN][KP];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int g = lane >> 4, r16 = lane & 15;
  // column blocks of one row group sit in adjacent blocks (blockIdx.x = group * ncb + cb; the grid
  // is a multiple of ncb), so the second column block's x rows are L2 hits
  const int ncb = (N + BN - 1) / BN;
  const int n0 = static_cast<int>(blockIdx.x % ncb) * BN;
  constexpr int AV = BF ? 8 : 4;  // A values per lane per fragment
  // fp32 x is loaded as float4s (16-B rows suffice); bf16 x as one 16-B load of 8 values
  constexpr int AVL = sizeof(TA) == 4 ? 4 : 8;
  const bool avec = (ldx % AVL == 0) && aligned(x, sizeof(TA) * AVL);
  const bool wvec = (ldwt % WV == 0) && aligned(wt, 16);
  const int64_t n_groups = (M + 127) / 128;
  const bool one_chunk = K <= KC;
  const bool vstore = vec_store && ldo % 4 == 0 && aligned(out, 16);  // 16-B output rows

  auto stage = [&](int kc) {
    if (wvec) {
      for (int e = t; e < BN * (KC / WV); e += kBlock) {
        const int n = e / (KC / WV), kv = (e - n * (KC / WV)) * WV;
        const int nn = n0 + n, k = kc + kv;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (nn < N && k + WV <= K) {
          v = *reinterpret_cast<const uint4*>(wt + static_cast<int64_t>(nn) * ldwt + k);
        } else if (nn < N && k < K) {
          WT tmp[WV];
#pragma unroll
          for (int q = 0; q < WV; ++q) tmp[q] = (k + q < K) ? wt[static_cast<int64_t>(nn) * ldwt + k + q] : WT(0);
          v = *reinterpret_cast<const uint4*>(tmp);
        }
        *reinterpret_cast<uint4*>(&Bt[n][kv]) = v;
      }
    } else {
      for (int e = t; e < BN * KC; e += kBlock) {
        const int n = e / KC, kk = e - n * KC;
        const int nn = n0 + n, k = kc + kk;
        Bt[n][kk] = (nn < N && k < K) ? wt[static_cast<int64_t>(nn) * ldwt + k] : WT(0);
      }
    }
  };
  if (one_chunk) {
    stage(0);
    __syncthreads();
  }
  for (int64_t grp = blockIdx.x / ncb; grp < n_groups; grp += gridDim.x / ncb) {
    const int64_t mw = grp * 128 + wv * 32;
    const TA* ap[2];
    bool aok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = mw + 16 * i + r16;
      aok[i] = m < M;
      const int64_t src = aok[i] ? (row_idx ? static_cast<int64_t>(row_idx[m]) : m) : 0;
      ap[i] = x + src * ldx;
    }
    f32x4 acc[2][NT];
    zero_tile(acc);

    for (int kc = 0; kc < K; kc += KC) {
      if (!one_chunk) {
        stage(kc);
        __syncthreads();
      }
      const int kend = (K - kc < KC) ? K - kc : KC;
      auto load_a = [&](int ks, float (&av)[2][AV]) {
        const int k0 = kc + ks + AV * g;  // first k of this lane's fragment
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if constexpr (sizeof(TA) == 4) {
            if (avec) {  // float4 pieces; a piece past K (K % 4 == 0) or past M reads zeros
#pragma unroll
              for (int q = 0; q < AV / 4; ++q) {
                const int kq = k0 + 4 * q;
                float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (aok[i] && kq + 4 <= K) {
                  v4 = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(ap[i]) + kq);
                } else if (aok[i] && kq < K) {
                  const float* pr = reinterpret_cast<const float*>(ap[i]) + kq;
                  v4.x = pr[0];
                  if (kq + 1 < K) v4.y = pr[1];
                  if (kq + 2 < K) v4.z = pr[2];
                }
                av[i][4 * q] = v4.x; av[i][4 * q + 1] = v4.y; av[i][4 * q + 2] = v4.z; av[i][4 * q + 3] = v4.w;
              }
              continue;
            }
          } else {
            if (avec && aok[i] && k0 + AV <= K) {  // bf16 x: one 16-B piece of 8 values
              const uint4 u = *reinterpret_cast<const uint4*>(ap[i] + k0);
              const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                av[i][2 * q] = __uint_as_float(uw[q] << 16);
                av[i][2 * q + 1] = __uint_as_float(uw[q] & 0xffff0000u);
              }
              continue;
            }
          }
#pragma unroll
          for (int q = 0; q < AV; ++q) {  // unaligned rows, a bf16 piece across K, rows past M: per element
            float v = 0.f;
            if (aok[i] && k0 + q < K) {
              if constexpr (sizeof(TA) == 4) v = reinterpret_cast<const float*>(ap[i])[k0 + q];
              else v = __uint_as_float(static_cast<uint32_t>(reinterpret_cast<const uint16_t*>(ap[i])[k0 + q]) << 16);
            }
            av[i][q] = v;
          }
        }
      };
      float avn[2][AV];
      if (PF) load_a(0, avn);
#pragma unroll 1
      for (int ks = 0; ks < kend; ks += KS) {
        float av[2][AV];
        if (PF) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < AV; ++q) av[i][q] = avn[i][q];
          if (ks + KS < kend) load_a(ks + KS, avn);
        } else {
          load_a(ks, av);
        }
        if constexpr (BF) {
          bf16x8 a8[2];
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 8; ++q) a8[i][q] = static_cast<short>(to_bf16_bits(av[i][q]));
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            const bf16x8 b8 = *reinterpret_cast<const bf16x8*>(&Bt[16 * c + r16][ks + 8 * g]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
              acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a8[i], b8, acc[i][c], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int c = 0; c < NT; ++c) {
            const float4 b4 = *reinterpret_cast<const float4*>(&Bt[16 * c + r16][ks + 4 * g]);
            const float bj[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int i = 0; i < 2; ++i)
                acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][j], bj[j], acc[i][c], 0, 0, 0);
          }
        }
      }
      if (!one_chunk) __syncthreads();
    }
    // store_tile's text, written out: through the helper k_mm_rows<float, float, 8, true> gained
    // 8 B of scratch and 15 spill instructions; this is the code the kernel had
    sf_tile(sf, acc);
    if (vstore) {
      // lane (g, r16 = 4q + p) holds C[4g + r][4q + p], r = 0..3; a 4x4 transpose inside each
      // lane quad (DPP swaps of lane bit 0, then bit 1) leaves C[4g + p][4q + r] -- four
      // consecutive columns of one row -- for one 16-B store instead of four dword stores
      const int p = r16 & 3, q = r16 >> 2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i][c][r];
#pragma unroll
          for (int m2 = 0; m2 < 2; ++m2) {  // bit 0: registers (2m2, 2m2+1) across lanes (p, p^1)
            const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2]), 0xB1, 0xF, 0xF, false));
            const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2 + 1]), 0xB1, 0xF, 0xF, false));
            if (p & 1) v[2 * m2] = sb; else v[2 * m2 + 1] = sa;
          }
#pragma unroll
          for (int m2 = 0; m2 < 2; ++m2) {  // bit 1: registers (m2, m2+2) across lanes (p, p^2)
            const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2]), 0x4E, 0xF, 0xF, false));
            const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2 + 2]), 0x4E, 0xF, 0xF, false));
            if (p & 2) v[m2] = sb; else v[m2 + 2] = sa;
          }
          const int64_t m = mw + 16 * i + 4 * g + p;
          const int n = n0 + 16 * c + 4 * q;
          if (m < M) {
            if (n + 3 < N) {
              *reinterpret_cast<float4*>(out + m * ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n + r < N) out[m * ldo + n + r] = v[r];
            }
          }
        }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t m = mw + 16 * i + 4 * g + r;
            const int n = n0 + 16 * c + r16;
            if (m < M && n < N) out[m * ldo + n] = acc[i][c][r];
          }
    }
  }
}

// fp32 UPDATE on MFMA with an LDS-DMA ring (the plain fp32 GEMM of GCN/GAT/SAGE layers,
// `template/ISA_defination.yaml:1-31` j,ij->i; LOAD_W `code/interpreter.py:335-343`).
// Why not k_mm_rows: there each K chunk of W is staged synchronously (stage, barrier, compute)
// and A fragments are loaded one 16-k step ahead, so at 4 waves per SIMD the MFMA pipe waits on
// HBM latency (61 TF/s of 157 at K = 602).  Here both operands go global -> LDS by
// global_load_lds (no VGPR staging), D 16-k stages deep, so every stage has D - 1 MFMA steps of
// other stages to land:
//   block = 4 waves = 64*FR rows x BN = 16*NT columns; per 16-k stage wave w DMAs its own FR
//   16-row A fragments (lane L = 16g + r holds x[row r][k0 + 4g .. +3], exactly the lane's MFMA
//   fragment, so the ds_read is lane-linear: conflict-free; the DMA takes 16-B pieces at the 4-B /
//   8-B aligned row starts of K = 602 / 1433 too) and NT/4 of the block's NT B fragments (W^T
//   rows, same layout);
//   per stage: counted s_waitcnt vmcnt (this wave's stage landed; the later stages stay in
//   flight), lgkmcnt(0) (this wave's reads of the slot about to be refilled are done), raw s_barrier
//   (every wave's DMA of the stage landed, every wave done with the old slot), then the DMA of
//   stage s + D - 1 and the 16-k MFMA step of stage s (FR x NT x 4 v_mfma_f32_16x16x4_f32).
// A K tail (K % 16) is one last step from registers with masked loads.  Rows past M and columns
// past N read clamped rows and are not stored.  Same per-lane k order and fma chain as
// k_mm_rows: results bitwise equal to it.  LDS: D x (4 FR + NT) KiB.
//   D = 3: the persistent many-group form (48 KiB at FR = 2, N = 128: 3 blocks per CU);
//   D = 4: the split-K form (one (row group, K slice) per block, three blocks per CU at FR = 1).
//   Deeper rings at fewer blocks per CU measured slower on every shape
//   (profiles/r03/mm_depth_sweep.log, mm_cora_epilogue.log) and are not built.
// Split K (kslice > 0): block row y contracts k in [y * kslice, +kslice) into output slice y.
// generic -> LDS address space, and the 32-bit LDS byte address (macros: a __device__ helper
// taking or returning address-space-3 pointers keeps hipcc from emitting a template kernel's host stub)
#define GTA_TO_LDS(p) ((__attribute__((address_space(3))) void*)(p))
#define GTA_LDS_ADDR(p) static_cast<uint32_t>(reinterpret_cast<uintptr_t>(GTA_TO_LDS(p)))
template <int OFF>
__device__ __forceinline__ void ds_read16(f32x4& v, uint32_t a) {  // result valid after an lgkmcnt wait
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(a), "i"(OFF));
}
__device__ __forceinline__ void ds_read16_kib(f32x4& v, uint32_t a, int c) {  // c: KiB offset < 64 (unrolled)
  switch (c) {
#define GTA_DSR(C_) case C_: ds_read16<(C_) * 1024>(v, a); break;
    GTA_DSR(0) GTA_DSR(1) GTA_DSR(2) GTA_DSR(3) GTA_DSR(4) GTA_DSR(5) GTA_DSR(6) GTA_DSR(7)
    GTA_DSR(8) GTA_DSR(9) GTA_DSR(10) GTA_DSR(11) GTA_DSR(12) GTA_DSR(13) GTA_DSR(14) GTA_DSR(15)
    GTA_DSR(16) GTA_DSR(17) GTA_DSR(18) GTA_DSR(19) GTA_DSR(20) GTA_DSR(21) GTA_DSR(22) GTA_DSR(23)
    GTA_DSR(24) GTA_DSR(25) GTA_DSR(26) GTA_DSR(27) GTA_DSR(28) GTA_DSR(29) GTA_DSR(30) GTA_DSR(31)
    GTA_DSR(32) GTA_DSR(33) GTA_DSR(34) GTA_DSR(35) GTA_DSR(36) GTA_DSR(37) GTA_DSR(38) GTA_DSR(39)
    GTA_DSR(40) GTA_DSR(41) GTA_DSR(42) GTA_DSR(43) GTA_DSR(44) GTA_DSR(45) GTA_DSR(46) GTA_DSR(47)
    GTA_DSR(48) GTA_DSR(49) GTA_DSR(50) GTA_DSR(51) GTA_DSR(52) GTA_DSR(53) GTA_DSR(54) GTA_DSR(55)
    GTA_DSR(56) GTA_DSR(57) GTA_DSR(58) GTA_DSR(59) GTA_DSR(60) GTA_DSR(61) GTA_DSR(62)
#undef GTA_DSR
    default: ds_read16<63 * 1024>(v, a); break;
  }
}
// s_waitcnt vmcnt(n * PS): everything but the last n stages of PS DMA instructions landed (n wave-uniform)
template <int PS>
__device__ __forceinline__ void vm_wait_stages(int n) {
  switch (n) {
#define GTA_VMW(N_) case N_: asm volatile("s_waitcnt vmcnt(%0)" ::"n"((N_) * PS) : "memory"); break;
    GTA_VMW(1) GTA_VMW(2) GTA_VMW(3) GTA_VMW(4) GTA_VMW(5) GTA_VMW(6)
#undef GTA_VMW
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}
// blocks per CU the ring's LDS allows (<= 4), the __launch_bounds__ waves per SIMD
constexpr int ring_blocks(int NT, int D, int FR) {
  return (160 / (D * (4 * FR + NT))) > 4 ? 4 : (160 / (D * (4 * FR + NT)));
}

// The persistent ring schedule, as k_mm_ring_bf runs it (k_mm_ring below keeps the same schedule
// written out: with these shared pieces its 64-row forms measured 5 - 11 % slower, DESIGN.md 3.8;
// until that cause is found RingSched and ring_run have this one caller).  A block's row groups
// are grp0, grp0 + gstep, ...; the ring runs on across them (stage t = (group j, step s) of S per
// group), so the next group's first stages land while this group finishes and no block pays a
// prologue after the first.  (j, s, slot) is the next stage to DMA as (group, stage in group, ring
// slot), advanced by one per issue: no 64-bit division per stage (its ~150 scalar instructions
// per stage were measurable).
template <int D>
struct RingSched {
  int64_t grp0, gstep, my_groups, T;  // T: this block's stages in all
  int S;
  int64_t j = 0;
  int s = 0, slot = 0;
  __device__ __forceinline__ RingSched(int ncb, int64_t n_groups, int S_)
      : grp0(blockIdx.x / ncb), gstep(gridDim.x / ncb),
        my_groups(grp0 < n_groups ? (n_groups - grp0 + gstep - 1) / gstep : 0), T(my_groups * S_), S(S_) {}
  __device__ __forceinline__ int64_t first_row(int64_t jj, int GR) const { return (grp0 + jj * gstep) * GR; }
  // one stage on; a kernel that sees j change recomputes its source rows (it compares j with the
  // group it holds rows of: a "new group" flag handed back from here cost registers and scratch)
  __device__ __forceinline__ void advance() {
    slot = slot + 1 == D ? 0 : slot + 1;
    if (++s == S) {
      s = 0;
      ++j;
    }
  }
};

// The ring's loop over this block's groups and stages.  issue() DMAs the stage at rs' cursor and
// advances it; stage(slot, s) reads stage s of the current group from its slot and runs its MFMA
// step; tail(j) adds a K tail the ring does not carry; epilogue(j) puts the group's rows out.
// Per stage: stage t landed (stages t+1 .. t+D-2 may stay in flight), every wave done with the
// slot about to be refilled (read at t-1), then the DMA of stage t + D - 1.
template <int PER_STAGE, int D, int FR, int NT, class Issue, class Stage, class Tail, class Epilogue>
__device__ __forceinline__ void ring_run(const RingSched<D>& rs, f32x4 (&acc)[FR][NT], Issue&& issue, Stage&& stage,
                                         Tail&& tail, Epilogue&& epilogue) {
  const int64_t T = rs.T, my_groups = rs.my_groups;
  const int S = rs.S;
  zero_tile(acc);  // (a slice shorter than one stage has no stages: T = 0, the tail does it all)
#pragma unroll
  for (int p = 0; p + 1 < D; ++p)
    if (p < T) issue();
  int64_t t = 0;
  int slot = 0;  // ring slot of stage t
  for (int64_t j = 0; j < my_groups; ++j) {
    for (int s = 0; s < S; ++s, ++t, slot = slot + 1 == D ? 0 : slot + 1) {
      const int64_t later = T - 1 - t;
      vm_wait_stages<PER_STAGE>(static_cast<int>(later < D - 2 ? later : D - 2));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (t + D - 1 < T) issue();
      stage(slot, s);
    }
    // the group's last stage is done: its K tail, its rows out, the next group's sums
    tail(j);
    epilogue(j);
    zero_tile(acc);
    // the counted waits above assume only ring DMA is outstanding; stores may retire out of order
    // with the loads, so drain them here (the next group's first stages have had a step to land)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// One 32-k bf16 step against W^T resident in LDS (stage_wt_frags' layout): the NT column fragments
// first_frag + c * frag_stride, in KiB from lds_addr (which carries the lane's 16-B offset), read,
// waited for and pinned, then NT x FR v_mfma_f32_16x16x32_bf16.  The A fragments a (16 B each: bf16x8,
// or the raw f32x4 of an LDS read issued just before the call) are pinned under the same wait and
// read as bf16x8 only after it.
template <int FR, int NT, typename A>
__device__ __forceinline__ void mma_bf_resident(f32x4 (&acc)[FR][NT], A (&a)[FR], uint32_t lds_addr, int first_frag,
                                                int frag_stride) {
  static_assert(sizeof(A) == 16, "one 16-B MFMA operand per fragment");
  f32x4 b4[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) ds_read16_kib(b4[c], lds_addr, first_frag + c * frag_stride);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < FR; ++i) asm volatile("" : "+v"(a[i]));
#pragma unroll
  for (int c = 0; c < NT; ++c) asm volatile("" : "+v"(b4[c]));
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    const bf16x8 b8 = __builtin_bit_cast(bf16x8, b4[c]);
#pragma unroll
    for (int i = 0; i < FR; ++i)
      acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[i]), b8, acc[i][c], 0, 0, 0);
  }
}

// W^T [N, K] bf16 into LDS in MFMA fragment layout, by every thread of the block (the caller's
// __syncthreads() publishes it): fragment (c, s) of NT x SB at dst + (c * SB + s) KiB holds lane L's
// 8 bf16 of row n0 + 16c + (L & 15), k = 32s + 8(L >> 4) .. +7, zeros past K and N.  A 16-B load
// where the piece is aligned and inside K, per element otherwise.
template <int NT, int SB>
__device__ __forceinline__ void stage_wt_frags(char* dst, const uint16_t* __restrict__ wt, int64_t ldwt, int n0, int N,
                                               int K) {
  for (int e = threadIdx.x; e < NT * SB * kWave; e += kBlock) {
    const int L = e & (kWave - 1), f = e >> 6, c = f / SB, s = f - c * SB;
    const int n = n0 + 16 * c + (L & 15), k = 32 * s + 8 * (L >> 4);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n < N && k < K) {
      const uint16_t* p = wt + static_cast<int64_t>(n) * ldwt + k;
      if (k + 8 <= K && aligned(p, 16)) {
        v = *reinterpret_cast<const uint4*>(p);
      } else {
        uint16_t tmp[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) tmp[q] = (k + q < K) ? p[q] : static_cast<uint16_t>(0);
        v = *reinterpret_cast<const uint4*>(tmp);
      }
    }
    *reinterpret_cast<uint4*>(dst + f * 1024 + L * 16) = v;
  }
}

template <int NT, int D = 3, int FR = 2>
__global__ void __launch_bounds__(kBlock, ring_blocks(NT, D, FR))
k_mm_ring(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ row_idx, int64_t M, int K,
          const float* __restrict__ wt, int64_t ldwt, int N, int sf, float* __restrict__ out, int64_t ldo,
          int kslice = 0, int64_t slice_stride = 0) {
  static_assert(NT == 4 || NT == 8, "B fragments split evenly over the 4 waves");
  static_assert(FR == 1 || FR == 2, "one or two A fragments per wave");
  static_assert(D >= 3 && D <= 8, "ring depth");
  if (kslice > 0) {
    const int k0 = static_cast<int>(blockIdx.y) * kslice;
    x += k0;
    wt += k0;
    K = min(kslice, K - k0);
    out += static_cast<int64_t>(blockIdx.y) * slice_stride;
  }
  constexpr int KS = 16, BN = 16 * NT, GR = 64 * FR;  // GR: rows per group
  // stage image: A [wave][i] then B [c], 1 KiB fragments (16 rows x 16 k)
  constexpr int A_BYTES = 4 * FR * 1024, STAGE = A_BYTES + NT * 1024;
  constexpr int PER_STAGE = FR + NT / 4;  // DMA instructions per wave per stage
  __shared__ __attribute__((aligned(16))) char lds[D * STAGE];
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = wave_id_uniform();
  const int g = lane >> 4, r16 = lane & 15;
  const int ncb = (N + BN - 1) / BN;
  const int n0 = static_cast<int>(blockIdx.x % ncb) * BN;
  // persistent: this block's row groups are grp0, grp0 + gstep, ...; the ring runs on across
  // them (stage t = (group j, 16-k step s)), so the next group's first stages land while this
  // group finishes and no block pays a prologue after the first
  const int64_t grp0 = blockIdx.x / ncb, gstep = gridDim.x / ncb;
  const int64_t n_groups = (M + GR - 1) / GR;
  const int64_t my_groups = grp0 < n_groups ? (n_groups - grp0 + gstep - 1) / gstep : 0;
  // stages per group: with K % 4 == 0 a K tail is one more ring stage whose 16-B pieces lie wholly
  // inside or wholly past K (those read the row start instead and are zeroed after the LDS read);
  // otherwise the tail is a register step of 16 k with masked loads, paid synchronously per group
  const bool ring_tail = (K % KS) != 0 && (K % 4) == 0;
  const int S = ring_tail ? (K + KS - 1) / KS : K / KS;
  // DMA lane map (row-contiguous): lane L fills row rr = L / 4 of a fragment with its 16-B piece
  // cp = L % 4, so 4 consecutive lanes read one row's 64 contiguous bytes; the piece it carries is
  // the logical k piece c = cp ^ ((rr >> 2) & 2), an XOR swizzle that keeps the fragment reads
  // below conflict-free in every ds_read_b128 lane group.  Lane (g, r) then reads logical piece g
  // of row r: the values and k order of the former lane = fragment map (lane (g, r) DMAing its own
  // piece: 16 rows per 16 consecutive lanes), bitwise equal and 1-4 % faster on every shape
  // measured (profiles/r03/mm_dma_rows_ab.log).
  const int rr = lane >> 2;
  const int cdma = (lane & 3) ^ ((rr >> 2) & 2);  // logical 16-B k piece this lane DMAs
  const uint32_t rdoff = static_cast<uint32_t>(r16 * 64 + ((g ^ ((r16 >> 2) & 2)) * 16));
  const bool dead = ring_tail && (S - 1) * KS + 4 * cdma >= K;  // this lane's DMA piece of the last stage
  const bool dead_rd = ring_tail && (S - 1) * KS + 4 * g >= K;  // the piece this lane reads
  const int64_t T = my_groups * S;
  const float* bsrc[NT / 4];
#pragma unroll
  for (int t = 0; t < NT / 4; ++t) {
    const int n = min(n0 + 16 * (wv * (NT / 4) + t) + rr, N - 1);
    bsrc[t] = wt + static_cast<int64_t>(n) * ldwt + 4 * cdma;
  }
  // A source row of group j, fragment i, fragment row sub
  auto a_row = [&](int64_t j, int i, int sub) __attribute__((always_inline)) -> const float* {
    const int64_t m = min<int64_t>((grp0 + j * gstep) * GR + wv * (16 * FR) + 16 * i + sub, M - 1);
    return x + (row_idx ? static_cast<int64_t>(row_idx[m]) : m) * ldx;
  };
  const float* asrc[FR];
  int64_t asrc_j = -1;
  // the next stage to DMA as (group, stage in group, ring slot), advanced by one per call: no
  // 64-bit division per stage (its ~150 scalar instructions per stage were measurable)
  int64_t iss_j = 0;
  int iss_s = 0, iss_slot = 0;
  auto issue = [&]() __attribute__((always_inline)) {
    const int64_t j = iss_j;
    const int k = iss_s * KS;
    if (j != asrc_j) {
#pragma unroll
      for (int i = 0; i < FR; ++i) asrc[i] = a_row(j, i, rr) + 4 * cdma;
      asrc_j = j;
    }
    char* base = lds + iss_slot * STAGE;
    iss_slot = iss_slot + 1 == D ? 0 : iss_slot + 1;
    const int ko = (dead && iss_s == S - 1) ? -4 * cdma : k;  // a piece past K reads its row's start
    if (++iss_s == S) {
      iss_s = 0;
      ++iss_j;
    }
#pragma unroll
    for (int i = 0; i < FR; ++i)
      __builtin_amdgcn_global_load_lds(const_cast<float*>(asrc[i] + ko), GTA_TO_LDS(base + (wv * FR + i) * 1024), 16, 0,
                                       0);
#pragma unroll
    for (int q = 0; q < NT / 4; ++q)
      __builtin_amdgcn_global_load_lds(const_cast<float*>(bsrc[q] + ko),  // (a const source fails the host pass)
                                       GTA_TO_LDS(base + A_BYTES + (wv * (NT / 4) + q) * 1024), 16, 0, 0);
  };
  f32x4 acc[FR][NT];
  auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto mma = [&](const float (&av)[FR][4], const float4& b4, int c) {
    const float bj[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < FR; ++i) acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][j], bj[j], acc[i][c], 0, 0, 0);
  };
  const bool vstore = ldo % 4 == 0 && aligned(out, 16);
  auto epilogue = [&](int64_t j) __attribute__((always_inline)) {
    const int64_t mw = (grp0 + j * gstep) * GR + wv * (16 * FR);
    sf_tile(sf, acc);
    if (vstore) {  // quad-transposed 16-B row stores (k_mm_rows' epilogue)
      const int p = r16 & 3, q = r16 >> 2;
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int c = 0; c < NT; ++c) {
          float v[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = acc[i][c][r];
#pragma unroll
          for (int m2 = 0; m2 < 2; ++m2) {
            const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2]), 0xB1, 0xF, 0xF, false));
            const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[2 * m2 + 1]), 0xB1, 0xF, 0xF, false));
            if (p & 1) v[2 * m2] = sb; else v[2 * m2 + 1] = sa;
          }
#pragma unroll
          for (int m2 = 0; m2 < 2; ++m2) {
            const float sa = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2]), 0x4E, 0xF, 0xF, false));
            const float sb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[m2 + 2]), 0x4E, 0xF, 0xF, false));
            if (p & 2) v[m2] = sb; else v[m2 + 2] = sa;
          }
          const int64_t m = mw + 16 * i + 4 * g + p;
          const int n = n0 + 16 * c + 4 * q;
          if (m < M) {
            if (n + 3 < N) {
              *reinterpret_cast<float4*>(out + m * ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (n + r < N) out[m * ldo + n + r] = v[r];
            }
          }
        }
    } else {
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t m = mw + 16 * i + 4 * g + r;
            const int n = n0 + 16 * c + r16;
            if (m < M && n < N) out[m * ldo + n] = acc[i][c][r];
          }
    }
  };
  auto tail = [&](int64_t j) __attribute__((always_inline)) {  // the K tail from registers, 16 k per step:
    for (int kt = S * KS; kt < K; kt += 16) {                     // k = kt + 4g + jj < K, zeros past it
      const int k0 = kt + 4 * g;
      auto ld4 = [&](const float* p) __attribute__((always_inline)) {  // p = row + k0
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 < K) v.x = p[0];
        if (k0 + 1 < K) v.y = p[1];
        if (k0 + 2 < K) v.z = p[2];
        if (k0 + 3 < K) v.w = p[3];
        return v;
      };
      float av[FR][4];
#pragma unroll
      for (int i = 0; i < FR; ++i) {
        const float4 a4 = ld4(a_row(j, i, r16) + k0);
        av[i][0] = a4.x; av[i][1] = a4.y; av[i][2] = a4.z; av[i][3] = a4.w;
      }
#pragma unroll
      for (int c = 0; c < NT; ++c) {
        const int n = min(n0 + 16 * c + r16, N - 1);
        mma(av, ld4(wt + static_cast<int64_t>(n) * ldwt + k0), c);
      }
    }
  };
  zero_acc();  // (a K < 16 slice has no stages: T = 0, the tail does it all)
#pragma unroll
  for (int p = 0; p + 1 < D; ++p)
    if (p < T) issue();
  int64_t t = 0;
  int slot = 0;  // ring slot of stage t
  for (int64_t j = 0; j < my_groups; ++j) {
  for (int s = 0; s < S; ++s, ++t, slot = slot + 1 == D ? 0 : slot + 1) {
    // stage t landed (stages t+1 .. t+D-2 may stay in flight), every wave done with the slot
    // about to be refilled (read at t-1)
    const int64_t later = T - 1 - t;
    vm_wait_stages<PER_STAGE>(static_cast<int>(later < D - 2 ? later : D - 2));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + D - 1 < T) issue();  // stage t + D - 1
    // fragment reads in inline asm: hipcc cannot tell them apart from the DMA in flight into
    // another slot and would wait vmcnt(0) before a plain LDS read (draining the ring every step).
    // The asm wait names every loaded register, so no MFMA is scheduled above it.
    const uint32_t sa = GTA_LDS_ADDR(lds + slot * STAGE + (wv * FR) * 1024) + rdoff;
    const uint32_t sb = GTA_LDS_ADDR(lds + slot * STAGE + A_BYTES) + rdoff;
    f32x4 a4[FR], b4[NT];
#pragma unroll
    for (int i = 0; i < FR; ++i) ds_read16_kib(a4[i], sa, i);
#pragma unroll
    for (int c = 0; c < NT; ++c) ds_read16_kib(b4[c], sb, c);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < FR; ++i) asm volatile("" : "+v"(a4[i]));
#pragma unroll
    for (int c = 0; c < NT; ++c) asm volatile("" : "+v"(b4[c]));
    if (dead_rd && s == S - 1) {  // pieces past K: zeros, as k_mm_rows' masked loads and staging give
#pragma unroll
      for (int i = 0; i < FR; ++i) a4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NT; ++c) b4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // j outermost: the FR x NT accumulators are each touched once per FR*NT MFMAs; per
    // accumulator the k order is k_mm_rows' (bitwise equal)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int i = 0; i < FR; ++i)
          acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[i][jj], b4[c][jj], acc[i][c], 0, 0, 0);
  }
  // the group's last stage is done: its K tail, its rows out, the next group's sums
  if (!ring_tail && (K % KS)) tail(j);
  epilogue(j);
  zero_acc();
  // the counted waits above assume only ring DMA is outstanding; stores may retire out of order
  // with the loads, so drain them here (the next group's first stages have had a step to land)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// fp32 UPDATE with one independent wave per block and no LDS (knob mm_wave): the same product as
// k_mm_ring -- `template/ISA_defination.yaml:1-31` j,ij->i, LOAD_W `code/interpreter.py:335-343` --
// without its per-stage block barrier.  A wave owns a (16 FR) x (16 NT) output tile and streams
// both operands straight into registers: per 16-k stage, lane L = 16g + r loads x[row r][k0 + 4g ..
// +3] of each of its FR row fragments and W^T[col r][k0 + 4g .. +3] of each of its NT column
// fragments (16-B buffer loads; the stage offset k0 * 4 is the scalar soffset), exactly its MFMA
// fragments, so nothing is staged or shuffled.  Step t issues W^T of stage t + 1, then x of stage
// t + 3, waits until stage t has landed and runs FR x NT x 4 v_mfma_f32_16x16x4_f32 on it: x (HBM)
// gets three stages of MFMA time to arrive, W^T (L2-resident) one.  The loads and the counted waits
// are inline asm in a fixed order -- with the intrinsics, the compiler sank every load to one stage
// ahead of its use (the registers it saved were not the bound), which left ~2 us of HBM latency
// exposed per 1.7 us stage.  The K tail is one more stage whose lanes past K are zeroed (loads past
// the tensor read 0 through the buffer bounds); stages past the last re-read it.  Same
// per-accumulator k order and fma chain as k_mm_rows / k_mm_ring: bitwise equal to them.
__device__ __forceinline__ void buf_load16(f32x4& v, uint32_t voff, const i32x4_t& rs, int soff) {
  asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
template <int NT, int FR, int WPS>
__global__ void __launch_bounds__(kWave, WPS)
k_mm_wave(const float* __restrict__ x, int64_t ldx, int64_t M, int K, const float* __restrict__ wt, int64_t ldwt, int N,
          int sf, float* __restrict__ out, int64_t ldo, uint32_t x_bytes, uint32_t w_bytes) {
  constexpr int GR = 16 * FR, BN = 16 * NT;
  const int lane = threadIdx.x;
  const int g = lane >> 4, r16 = lane & 15;
  const int ncb = (N + BN - 1) / BN;
  const int64_t n_units = (M + GR - 1) / GR * ncb;
  const i32x4_t rx = buf_desc(x, x_bytes), rw = buf_desc(wt, w_bytes);
  const int SF = (K + 15) / 16;  // stages, the K tail included
  const bool tail = (K & 15) != 0;
  const bool vstore = ldo % 4 == 0 && aligned(out, 16);
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int n0 = static_cast<int>(u % ncb) * BN;
    const int64_t mw = u / ncb * GR;
    uint32_t ao[FR], bo[NT];
#pragma unroll
    for (int i = 0; i < FR; ++i)
      ao[i] = static_cast<uint32_t>((min<int64_t>(mw + 16 * i + r16, M - 1) * ldx + 4 * g) * 4);
#pragma unroll
    for (int c = 0; c < NT; ++c) bo[c] = static_cast<uint32_t>((static_cast<int64_t>(min(n0 + 16 * c + r16, N - 1)) * ldwt + 4 * g) * 4);
    f32x4 acc[FR][NT];
    zero_tile(acc);
    f32x4 a0[FR], a1[FR], a2[FR], a3[FR], b0[NT], b1[NT];
    auto load_a = [&](f32x4 (&a)[FR], int s) __attribute__((always_inline)) {
      const int so = min(s, SF - 1) * 64;
#pragma unroll
      for (int i = 0; i < FR; ++i) buf_load16(a[i], ao[i], rx, so);
    };
    auto load_b = [&](f32x4 (&b)[NT], int s) __attribute__((always_inline)) {
      const int so = min(s, SF - 1) * 64;
#pragma unroll
      for (int c = 0; c < NT; ++c) buf_load16(b[c], bo[c], rw, so);
    };
    // step t: W^T of t + 1 into bn, x of t + 3 into an; then stage t (ac, bc) has landed once at most
    // the loads issued after B(t) -- x of t + 2 (the step before), bn and an -- are outstanding
    auto step = [&](f32x4 (&ac)[FR], f32x4 (&bc)[NT], f32x4 (&bn)[NT], f32x4 (&an)[FR], int t)
        __attribute__((always_inline)) {
      load_b(bn, t + 1);
      load_a(an, t + 3);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * FR + NT) : "memory");
#pragma unroll
      for (int i = 0; i < FR; ++i) asm volatile("" : "+v"(ac[i]));
#pragma unroll
      for (int c = 0; c < NT; ++c) asm volatile("" : "+v"(bc[c]));
      if (tail && t == SF - 1) {  // k = 16 t + 4 g + e past K: zero (as k_mm_rows' masked loads)
        const int k0 = 16 * t + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool past = k0 + e >= K;
#pragma unroll
          for (int i = 0; i < FR; ++i) ac[i][e] = past ? 0.f : ac[i][e];
#pragma unroll
          for (int c = 0; c < NT; ++c) bc[c][e] = past ? 0.f : bc[c][e];
        }
      }
      mma_f32_step(acc, ac, bc);
    };
    // issue order A(0), A(1), B(0), A(2): after B(t) come A(t + 2), B(t + 1), A(t + 3) for every t
    load_a(a0, 0);
    load_a(a1, 1);
    load_b(b0, 0);
    load_a(a2, 2);
    int t = 0;  // a0..a2 hold stages t..t + 2, b0 stage t
    for (; t + 4 <= SF; t += 4) {
      step(a0, b0, b1, a3, t);
      step(a1, b1, b0, a0, t + 1);
      step(a2, b0, b1, a1, t + 2);
      step(a3, b1, b0, a2, t + 3);
    }
    // nested, so the control-flow graph holds only the feasible paths (a third step always follows
    // the first two): asmcheck.py's path-insensitive wait analysis then proves every operand landed
    const int rem = SF - t;
    if (rem >= 1) {
      step(a0, b0, b1, a3, t);
      if (rem >= 2) {
        step(a1, b1, b0, a0, t + 1);
        if (rem >= 3) step(a2, b0, b1, a1, t + 2);
      }
    }
    // the loads issued past the last stage, and the stores below, drained before the next unit
    // counts its own loads
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ... and every load target kept live until that wait: a stage loaded past the end is dead, and
    // the compiler gave such registers to other values while the load was still in flight (a late
    // return then overwrote them; asmcheck.py found it in the remainder of k_mm_wave<8, 4, 1>)
#pragma unroll
    for (int i = 0; i < FR; ++i) asm volatile("" ::"v"(a0[i]), "v"(a1[i]), "v"(a2[i]), "v"(a3[i]));
#pragma unroll
    for (int c = 0; c < NT; ++c) asm volatile("" ::"v"(b0[c]), "v"(b1[c]));
    sf_tile(sf, acc);
    store_tile(acc, out, ldo, M, N, mw, n0, lane, vstore);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// bf16 MFMA UPDATE with an LDS-DMA ring (GTA_F32_BF16: fp32 x rounded to bf16 as it leaves LDS,
// bf16 W; GTA_BF16: bf16 x and W) -- the GIN MLP GEMMs [2.45 M x 100].[100 x 128] and
// [2.45 M x 128].[128 x 128] (`vTCAD/GraphOP/genGraphOP.py:97-108`, applynode MM
// `template/ISA_defination.yaml:1-31`).  These are HBM-bound streams (x read once, out written
// once, ~2 GFLOP per GB), so what matters is bytes in flight: x goes global -> LDS by
// global_load_lds through a D-deep ring of 32-k stages (lane L = 16g + r holds x[row r][k0 + 8g
// .. +7], its own MFMA fragment: two 16-B pieces for fp32 x, one for bf16), while W^T -- at most
// SB 32-k steps x BN columns, 32 KiB at K <= 128 -- is staged once per block into LDS in the same
// fragment layout, zero past K and N.  Per stage: counted vmcnt + raw s_barrier as in k_mm_ring,
// FR x NT v_mfma_f32_16x16x32_bf16 per wave.  A K tail (K % 32) is one register step with masked
// loads.  Same k order, the same RNE rounding of x (to_bf16_bits) and the same zero padding as
// k_mm_rows: results bitwise equal to it.
constexpr int ring_bf_blocks(int NT, int D, int FR, int SB, int PA) {  // blocks per CU its LDS allows (<= 4)
  return (160 / (D * 4 * FR * PA + NT * SB)) > 4 ? 4 : (160 / (D * 4 * FR * PA + NT * SB));
}

template <typename TA, int NT, int D = 3, int FR = 2, int SB = 4>
__global__ void __launch_bounds__(kBlock, ring_bf_blocks(NT, D, FR, SB, sizeof(TA) == 4 ? 2 : 1))
k_mm_ring_bf(const TA* __restrict__ x, int64_t ldx, const int32_t* __restrict__ row_idx, int64_t M, int K,
             const uint16_t* __restrict__ wt, int64_t ldwt, int N, int sf, float* __restrict__ out, int64_t ldo) {
  static_assert(NT == 4 || NT == 8, "column fragments");
  static_assert(FR == 1 || FR == 2, "one or two A fragments per wave");
  static_assert(D >= 3 && D <= 8, "ring depth");
  constexpr int KS = 32, BN = 16 * NT, GR = 64 * FR;
  constexpr int PA = sizeof(TA) == 4 ? 2 : 1;  // 16-B DMA pieces per lane per A fragment
  constexpr int FRAG = PA * 1024, STAGE = 4 * FR * FRAG;
  constexpr int PER_STAGE = FR * PA;           // DMA instructions per wave per stage
  __shared__ __attribute__((aligned(16))) char lds[D * STAGE];
  __shared__ __attribute__((aligned(16))) char bres[NT * SB * 1024];
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = wave_id_uniform();
  const int g = lane >> 4, r16 = lane & 15;
  const int ncb = (N + BN - 1) / BN;
  const int n0 = static_cast<int>(blockIdx.x % ncb) * BN;
  // a K tail is one more ring stage when its pieces (4 fp32 / 8 bf16) lie wholly inside or wholly past
  // K (those read the row start and are zeroed after the LDS read); else a masked register step
  const bool ring_tail = (K % KS) != 0 && (K % (PA == 2 ? 4 : 8)) == 0;
  const int S = ring_tail ? (K + KS - 1) / KS : K / KS;
  const int kdead = ring_tail ? K - (S - 1) * KS : KS;  // pieces of the last stage from this k (lane-relative) are past K
  RingSched<D> rs(ncb, (M + GR - 1) / GR, S);
  stage_wt_frags<NT, SB>(bres, wt, ldwt, n0, N, K);
  auto a_row = [&](int64_t j, int i, int sub) __attribute__((always_inline)) -> const TA* {
    const int64_t m = min<int64_t>(rs.first_row(j, GR) + wv * (16 * FR) + 16 * i + sub, M - 1);
    return x + (row_idx ? static_cast<int64_t>(row_idx[m]) : m) * ldx;
  };
  // DMA lane map (row-contiguous, as k_mm_ring's): DMA instruction p of a fragment holds rows
  // RPI p .. RPI p + RPI - 1 (RPI = 8 fp32 / 16 bf16), LPR consecutive lanes reading one row's 32-k
  // stage slice (128 / 64 contiguous bytes); lane L carries logical piece c = (L % LPR) ^ swz(row),
  // the XOR swizzle that keeps the fragment reads conflict-free in every ds_read_b128 lane group.
  // The image holds a fragment's rows in order ([16][RB] bytes) and lane (g, r) reads logical piece
  // 2g + p (fp32) / g (bf16) of row r: the values and k order of the lane = fragment map.
  constexpr int RB = 32 * static_cast<int>(sizeof(TA)), LPR = RB / 16, RPI = 64 / LPR;
  auto swz = [](int r) __attribute__((always_inline)) { return PA == 2 ? (r >> 1) & 5 : (r >> 2) & 2; };
  int drow[PA], doff[PA];  // per DMA instruction p: fragment row, element offset of the lane's piece
  uint32_t rdoff[PA];      // per read p: byte offset of logical piece (2g + p | g) of row r16
#pragma unroll
  for (int p = 0; p < PA; ++p) {
    drow[p] = RPI * p + lane / LPR;
    doff[p] = ((lane % LPR) ^ swz(drow[p])) * (16 / static_cast<int>(sizeof(TA)));
    rdoff[p] = static_cast<uint32_t>(r16 * RB + (((PA == 2 ? 2 * g + p : g)) ^ swz(r16)) * 16);
  }
  const TA* asrc[FR][PA];
  int64_t asrc_j = -1;  // the group asrc holds rows of
  auto issue = [&]() __attribute__((always_inline)) {  // the DMA of stage rs.(j, s) into rs.slot
    if (rs.j != asrc_j) {
      asrc_j = rs.j;
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int p = 0; p < PA; ++p) asrc[i][p] = a_row(rs.j, i, drow[p]) + doff[p];
    }
    char* base = lds + rs.slot * STAGE;
    const int k = rs.s * KS;
    const bool last = ring_tail && rs.s == S - 1;
    rs.advance();
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int p = 0; p < PA; ++p)
      {  // (a non-dependent source pointer: a TA-dependent builtin argument drops the kernel's host stub)
        const int ko = (last && doff[p] >= kdead) ? -doff[p] : k;  // a piece past K reads its row's start
        const char* src = reinterpret_cast<const char*>(asrc[i][p] + ko);
        __builtin_amdgcn_global_load_lds(const_cast<char*>(src), GTA_TO_LDS(base + (wv * FR + i) * FRAG + p * 1024), 16,
                                         0, 0);
      }
  };
  f32x4 acc[FR][NT];
  // 8 values of one lane's fragment -> the bf16x8 MFMA operand (fp32: RNE as k_mm_rows rounds)
  auto pack = [&](const float (&v)[8]) __attribute__((always_inline)) {
    bf16x8 r;
#pragma unroll
    for (int q = 0; q < 8; ++q) r[q] = static_cast<short>(to_bf16_bits(v[q]));
    return r;
  };
  const uint32_t bbase = GTA_LDS_ADDR(bres) + static_cast<uint32_t>(lane) * 16u;
  auto stage = [&](int slot, int s) __attribute__((always_inline)) {
    const uint32_t sa = GTA_LDS_ADDR(lds + slot * STAGE + (wv * FR) * FRAG);
    f32x4 a4[FR][PA];
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int p = 0; p < PA; ++p) ds_read16_kib(a4[i][p], sa + rdoff[p], i * PA);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int i = 0; i < FR; ++i)
#pragma unroll
      for (int p = 0; p < PA; ++p) asm volatile("" : "+v"(a4[i][p]));
    if (ring_tail && s == S - 1) {  // pieces past K: zeros, as k_mm_rows' masked loads give
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int p = 0; p < PA; ++p)
          if (8 * g + 4 * p >= kdead) a4[i][p] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    bf16x8 a8[FR];
#pragma unroll
    for (int i = 0; i < FR; ++i) {
      if constexpr (PA == 2) {
        const float v[8] = {a4[i][0][0], a4[i][0][1], a4[i][0][2], a4[i][0][3],
                            a4[i][1][0], a4[i][1][1], a4[i][1][2], a4[i][1][3]};
        a8[i] = pack(v);
      } else {
        a8[i] = __builtin_bit_cast(bf16x8, a4[i][0]);
      }
    }
    mma_bf_resident(acc, a8, bbase + static_cast<uint32_t>(s) * 1024u, 0, SB);
  };
  auto tail = [&](int64_t j) __attribute__((always_inline)) {  // k in [32 S, K): masked register step
    if (ring_tail || K % KS == 0) return;
    const int k0 = S * KS + 8 * g;
    bf16x8 a8[FR];
#pragma unroll
    for (int i = 0; i < FR; ++i) {
      const TA* p = a_row(j, i, r16) + k0;
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (k0 + q < K) ? load_elem(p + q) : 0.f;
      a8[i] = pack(v);
    }
    mma_bf_resident(acc, a8, bbase + static_cast<uint32_t>(S) * 1024u, 0, SB);
  };
  const bool vstore = ldo % 4 == 0 && aligned(out, 16);
  auto epilogue = [&](int64_t j) __attribute__((always_inline)) {
    sf_tile(sf, acc);
    store_tile(acc, out, ldo, M, N, rs.first_row(j, GR) + wv * (16 * FR), n0, lane, vstore);
  };
  __syncthreads();  // W^T resident before any fragment read
  ring_run<PER_STAGE>(rs, acc, issue, stage, tail, epilogue);
}

// Two chained node GEMMs in one pass (GIN's MLP, `vTCAD/GraphOP/genGraphOP.py:103-108`: applynode
// MM -> SF -> MM -> SF, `template/ISA_defination.yaml:1-31` j,ij->i twice):
//   out = sf2(bf16(sf1(x W1)) W2), x fp32 [M, K1 <= 128], W1 bf16 [K1, N1 <= 128], W2 bf16 [N1, N2 <= 128].
// The unfused path writes z = sf1(x W1) as fp32 [M, N1] and the second GEMM reads it back, rounding
// it to bf16 as it stages it (GTA_F32_BF16): 2 x M x N1 x 4 bytes of HBM traffic (2.5 GB for GIN
// products) that this kernel never moves -- x is read once and out written once.
// Per wave: 16-row groups, persistent.  x fragments go straight to registers (lane (g, r) loads
// x[r][32s + 8g .. +7] as two float4s, the next group's loads in flight during this group's
// MFMAs) and are rounded to bf16 (RNE) as k_mm_ring_bf rounds them; W1^T and W2^T stay resident in
// LDS in k_mm_ring_bf's fragment layout (zero past K and N).  GEMM 1 is NT x ceil(K1/32)
// v_mfma_f32_16x16x32_bf16 in k_mm_ring_bf's k order; its tile goes sf1 -> bf16 (RNE, as the
// second GEMM's staging rounds the fp32 z) -> the wave's own 16 x 128 bf16 LDS image (quad-transposed
// 8-B writes, 16-B pieces XOR-swizzled by row so the A-fragment reads are conflict-free) -> GEMM 2
// (4 steps of 32 k, zero past N1).  Same operands, k order and rounding as the two unfused
// launches: bitwise equal to them.  LDS 80 KiB: two blocks per CU.
// SF1 / SF2: the SFs as template constants (RELU / NONE: the GIN configurations), -1 = the runtime
// sf1 / sf2 (every other SF; a switch per tile).  x rows 16-B aligned with K1 % 4 == 0 (the host
// checks), so every 16-B piece of x is wholly inside K1 or wholly past it: clamped loads and a
// select, no branches -- a branchy masked load made the compiler drain every load in flight.
// TA = uint16_t: x is bf16 already (the aggregate rounded it, gta_aggregate_self y_dtype BF16): one
// 16-B piece of 8 values per lane and 32-k step, pairs past K1 zeroed; no rounding (exact values).
template <int SF1, int SF2, typename TA = float>
__global__ void __launch_bounds__(kBlock, 2)
k_mlp_bf(const TA* __restrict__ x, int64_t ldx, int64_t M, int K1, const uint16_t* __restrict__ w1t,
         int64_t ldw1, int N1, int sf1, const uint16_t* __restrict__ w2t, int64_t ldw2, int N2, int sf2,
         float* __restrict__ out, int64_t ldo) {
  constexpr int NT = 8, SB = 4;  // 128 columns, 128 k of resident W^T per GEMM
  __shared__ __attribute__((aligned(16))) char wres[2 * NT * SB * 1024];
  __shared__ __attribute__((aligned(16))) char zimg[kWavesPerBlock * 16 * 256];
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = wave_id_uniform();
  const int g = lane >> 4, r16 = lane & 15;
  // W1^T, W2^T resident: fragment (w, c, s) at wres + ((w * NT + c) * SB + s) KiB; zeros past K (W1:
  // K1, W2: N1) and N
  stage_wt_frags<NT, SB>(wres, w1t, ldw1, 0, N1, K1);
  stage_wt_frags<NT, SB>(wres + NT * SB * 1024, w2t, ldw2, 0, N2, N1);
  __syncthreads();
  const int64_t n_groups = (M + 15) / 16;
  const int64_t gstep = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  int64_t grp = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wv;
  // x pieces by buffer loads through a descriptor over the group's rows: a piece past K1 (or a row
  // past M) takes an out-of-range offset and reads zeros -- no branch around the loads, so nothing
  // makes the compiler drain the next groups' loads in flight.  fp32 x: two 16-B pieces per step;
  // bf16 x: one (held in xa[st][0]), its 4-B pairs past K1 zeroed by a select
  constexpr bool XB = sizeof(TA) == 2;
  const uint32_t row_bytes = static_cast<uint32_t>(ldx) * static_cast<uint32_t>(sizeof(TA));
  // The loads are inline asm in program order (with the intrinsics the compiler sank them next to
  // their use and drained every load in flight at each group); x_wait() below counts them.
  constexpr int LPG = XB ? SB : 2 * SB;  // loads per group
  auto load_x = [&](int64_t gi, f32x4 (&xa)[SB][2]) __attribute__((always_inline)) {
    const int64_t row0 = gi * 16;
    const int64_t rows = max<int64_t>(0, min<int64_t>(16, M - row0));  // 0 past the last group: all zeros
    const i32x4_t rs = buf_desc(x + row0 * ldx, static_cast<uint32_t>(rows * row_bytes));
    const uint32_t roff = static_cast<uint32_t>(r16) * row_bytes;
#pragma unroll
    for (int st = 0; st < SB; ++st) {
      if constexpr (XB) {
        const int k = 32 * st + 8 * g;
        buf_load16(xa[st][0], k < K1 ? roff + static_cast<uint32_t>(k) * 2u : 0x80000000u, rs, 0);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int k = 32 * st + 8 * g + 4 * h;
          buf_load16(xa[st][h], k < K1 ? roff + static_cast<uint32_t>(k) * 4u : 0x80000000u, rs, 0);
        }
      }
    }
  };
  // a group's x landed: at most the two later groups' loads are outstanding (stores are not counted:
  // they may retire out of order with the loads, and an outstanding one only makes the wait longer)
  auto x_wait = [&](f32x4 (&xa)[SB][2]) __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LPG) : "memory");
#pragma unroll
    for (int st = 0; st < SB; ++st) {
      asm volatile("" : "+v"(xa[st][0]));
      if constexpr (!XB) asm volatile("" : "+v"(xa[st][1]));
    }
    if constexpr (XB) {
#pragma unroll
      for (int st = 0; st < SB; ++st) {  // 4-B pairs past K1 zeroed (K1 is even: a pair is wholly in or past)
        const int k = 32 * st + 8 * g;
        uint4 v = __builtin_bit_cast(uint4, xa[st][0]);
        v.x = k < K1 ? v.x : 0u;
        v.y = k + 2 < K1 ? v.y : 0u;
        v.z = k + 4 < K1 ? v.z : 0u;
        v.w = k + 6 < K1 ? v.w : 0u;
        xa[st][0] = __builtin_bit_cast(f32x4, v);
      }
    }
  };
  auto sf_acc = [&](f32x4 (&acc)[1][NT], int sfc, auto tag) __attribute__((always_inline)) {
    constexpr int K = decltype(tag)::value;
    if constexpr (K < 0) {
      sf_tile(sfc, acc);
    } else if constexpr (K != GTA_SF_NONE) {
#pragma unroll
      for (int c = 0; c < NT; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[0][c][r] = sf_apply(K, acc[0][c][r]);
    }
  };
  const uint32_t wbase = GTA_LDS_ADDR(wres) + static_cast<uint32_t>(lane) * 16u;
  const uint32_t zw = GTA_LDS_ADDR(zimg) + static_cast<uint32_t>(wv) * 4096u;
  const bool vstore = ldo % 4 == 0 && aligned(out, 16);
  const int p = r16 & 3, qq = r16 >> 2;
  // one 16-row group: GEMM 1, the z image, GEMM 2, the stores
  auto compute = [&](const f32x4 (&xa)[SB][2], int64_t grp) __attribute__((always_inline)) {
    f32x4 acc[1][NT];
    zero_tile(acc);
    // GEMM 1: k_mm_ring_bf's step order, every step padded with zeros past K1
#pragma unroll
    for (int st = 0; st < SB; ++st) {
      if (32 * st >= K1) break;  // (wave-uniform)
      bf16x8 a8[1];  // x rounded to bf16 (RNE) as k_mm_ring_bf rounds it (a bf16 x: its own bits)
      if constexpr (XB) {
        a8[0] = __builtin_bit_cast(bf16x8, xa[st][0]);
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) a8[0][q] = static_cast<short>(to_bf16_bits(xa[st][q >> 2][q & 3]));
      }
      mma_bf_resident(acc, a8, wbase, st, SB);
    }
    sf_acc(acc, sf1, std::integral_constant<int, SF1>{});
    // z tile -> bf16 image [16 rows][128 k] of this wave: lane (g, 4qq + p) holds rows 4g + r, column
    // 16c + 4qq + p; the quad transpose leaves row 4g + p, columns 16c + 4qq .. +3 (one 8-B write).
    // 16-B piece P of row r sits at piece P ^ r (conflict-free A-fragment reads below)
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[0][c][r];
      quad_transpose(v, p);
      const int row = 4 * g + p, col = 16 * c + 4 * qq;  // columns past N1 are zero (K of GEMM 2)
      uint32_t lo = 0, hi = 0;
      if (col < N1) lo |= to_bf16_bits(v[0]);
      if (col + 1 < N1) lo |= static_cast<uint32_t>(to_bf16_bits(v[1])) << 16;
      if (col + 2 < N1) hi |= to_bf16_bits(v[2]);
      if (col + 3 < N1) hi |= static_cast<uint32_t>(to_bf16_bits(v[3])) << 16;
      const uint32_t a = zw + static_cast<uint32_t>(row * 256 + (((2 * c + (qq >> 1)) ^ row) * 16) + (qq & 1) * 8);
      asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(make_uint2(lo, hi)) : "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // GEMM 2: A fragment (row r16, k = 32 s + 8 g .. +7) = logical piece 4 s + g of row r16
    zero_tile(acc);
#pragma unroll
    for (int st = 0; st < SB; ++st) {
      f32x4 a4[1];  // (lands under mma_bf_resident's wait, which pins it before its first use)
      ds_read16<0>(a4[0], zw + static_cast<uint32_t>(r16 * 256 + (((4 * st + g) ^ r16) * 16)));
      mma_bf_resident(acc, a4, wbase, NT * SB + st, SB);
    }
    sf_acc(acc, sf2, std::integral_constant<int, SF2>{});
    store_tile(acc, out, ldo, M, N2, grp * 16, 0, lane, vstore);
  };
  // three register buffers, two groups' x loads in flight while one group computes (a group's MFMA
  // work is shorter than an HBM round trip; one group ahead left the waves waiting on their loads)
  // The loop body is straight-line (no exits between the loads and their use, which would let the
  // compiler sink the loads next to their use): every wave runs whole rounds of three groups, and a
  // group past the last reads zeros (empty descriptor) and stores nothing (rows past M are masked).
  const int64_t mine = grp < n_groups ? (n_groups - grp + gstep - 1) / gstep : 0;
  const int64_t rounds = (mine + 2) / 3;
  f32x4 xa[SB][2], xb[SB][2], xc[SB][2];
  if (rounds > 0) {
    load_x(grp, xa);
    load_x(grp + gstep, xb);
  }
  for (int64_t t = 0; t < rounds; ++t, grp += 3 * gstep) {
    load_x(grp + 2 * gstep, xc);
    x_wait(xa);
    compute(xa, grp);
    load_x(grp + 3 * gstep, xa);
    x_wait(xb);
    compute(xb, grp + gstep);
    load_x(grp + 4 * gstep, xb);
    x_wait(xc);
    compute(xc, grp + 2 * gstep);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the loads issued past the last group
}

// out[m, n] = sf(sum_s ws[s][m][n]) in slice order (split-K UPDATE; ws slices are [M, N] dense).
// Float4 form: four consecutive columns per thread, the slices' loads issued four at a time, the
// adds in slice order (bitwise equal to the scalar form).
__global__ void __launch_bounds__(kBlock)
k_mm_slices_sum(const float* __restrict__ ws, int S, int64_t M, int N, int sf, float* __restrict__ out, int64_t ldo) {
  const int64_t total = M * N;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float a = 0.f;
    for (int k = 0; k < S; ++k) a += ws[k * total + t];
    const int64_t m = t / N;
    out[m * ldo + (t - m * N)] = sf_apply(sf, a);
  }
}

__global__ void __launch_bounds__(kBlock)
k_mm_slices_sum4(const float4* __restrict__ ws, int S, int64_t M, int N4, int sf, float* __restrict__ out,
                 int64_t ldo) {
  const int64_t total4 = M * N4;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total4;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int k = 0;
    for (; k + 4 <= S; k += 4) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ws[(k + u) * total4 + t];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a.x += v[u].x; a.y += v[u].y; a.z += v[u].z; a.w += v[u].w;
      }
    }
    for (; k < S; ++k) {
      const float4 v = ws[k * total4 + t];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    const int64_t m = t / N4;
    *reinterpret_cast<float4*>(out + m * ldo + (t - m * N4) * 4) =
        make_float4(sf_apply(sf, a.x), sf_apply(sf, a.y), sf_apply(sf, a.z), sf_apply(sf, a.w));
  }
}

// ---------------------------------------------------------------------------
// f2: tile-nnz histogram (integer atomics: result is order independent)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_tile_nnz(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
           int64_t n_cols, int64_t T, int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  int32_t* base = counts + (row / T) * n_cols;
  const int64_t eb = indptr[row];
  for (int64_t e = eb + lane; e < indptr[row + 1]; e += kWave) {
    const int32_t j = indices[e];
    // a dense adjacency holds each (row, j) once: skip self loops and repeats of the previous column
    if (j != row && (e == eb || indices[e - 1] != j)) atomicAdd(base + j, 1);
  }
}

// ---------------------------------------------------------------------------
// Synthetic-workload setup (the bench's GAT alpha and CSR row ids), ABI 12.  One wave per row and
// no dependency between workgroups: no device-wide scan, sort or look-back, so a shard builds the
// same way whatever else shares the GPU (the 8-process one-GPU rehearsal stalled in
// torch's scan-based segment_reduce / repeat_interleave).
// ---------------------------------------------------------------------------
// graph.mix32 / graph.hash32: the lowbias32 counter hash, in uint32 arithmetic (the Python form
// masks to 32 bits at the same points, so the two agree bit for bit).
__host__ __device__ inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  return x ^ (x >> 16);
}

__host__ __device__ inline uint32_t hash_key(int64_t seed, int64_t stream) {  // key of graph.hash32, before mix32
  return static_cast<uint32_t>((static_cast<uint64_t>(seed) * 0x9E3779B9ull + static_cast<uint64_t>(stream) * 0x85EBCA6Bull +
                                0x27D4EB2Full) & 0xFFFFFFFFull);
}

// graph.hash_normal(idx, seed, stream) for one idx: Box-Muller in fp64 on two counter hashes, each
// operation rounded where torch rounds it (one kernel per op there), then one cast to fp32.
__device__ __forceinline__ float hash_normal1(uint64_t idx, uint32_t k1, uint32_t s1, uint32_t k2, uint32_t s2) {
  const uint32_t lo = static_cast<uint32_t>(idx);
  const uint32_t h1 = mix32(mix32(lo ^ k1) + s1), h2 = mix32(mix32(lo ^ k2) + s2);
  const double u1 = (static_cast<double>(h1) + 0.5) * (1.0 / 4294967296.0);
  const double u2 = static_cast<double>(h2) * (1.0 / 4294967296.0);
  const double r = sqrt(-2.0 * log(u1));
  const double c = cos(6.283185307179586 * u2);
  return static_cast<float>(r * c);
}

// alpha[e, h] = ex[e, h] / s[row(e), h], ex = exp(hash_normal(gen[e] * H + h)), s = the row's fp64
// sum of ex in edge order, cast to fp32 (metric.alpha_rows).  Lane = (edge slot e % (64 / H), head
// h); the serial sum runs in every lane of head h (shuffles from the slots in edge order), so it
// adds the same values in the same order as a one-thread-per-(row, head) loop.
__global__ void __launch_bounds__(kBlock)
k_synth_alpha(const int64_t* __restrict__ indptr, const int64_t* __restrict__ gen, int64_t n_rows, int H,
              uint32_t k1, uint32_t s1, uint32_t k2, uint32_t s2, float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int per = kWave / H, slot = lane / H, h = lane % H;
  const int64_t eb = indptr[row], ee = indptr[row + 1];
  double s = 0.0;
  for (int64_t e0 = eb; e0 < ee; e0 += per) {
    const int64_t e = e0 + slot;
    float ex = 0.f;
    if (e < ee) {
      ex = expf(hash_normal1(static_cast<uint64_t>(gen[e]) * static_cast<uint64_t>(H) + static_cast<uint64_t>(h), k1, s1,
                             k2, s2));
      out[e * H + h] = ex;
    }
    const int n = static_cast<int>(min<int64_t>(per, ee - e0));
    for (int j = 0; j < n; ++j) s += static_cast<double>(__shfl(ex, j * H + h));
  }
  const float sf = static_cast<float>(s);
  for (int64_t e = eb + slot; e < ee; e += per) out[e * H + h] = out[e * H + h] / sf;
}

// row id of every CSR edge (torch.repeat_interleave(arange(n_rows), degrees)), int64
__global__ void __launch_bounds__(kBlock)
k_row_ids(const int64_t* __restrict__ indptr, int64_t n_rows, int64_t* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  for (int64_t e = indptr[row] + lane; e < indptr[row + 1]; e += kWave) out[e] = row;
}

// ---------------------------------------------------------------------------
// host-side dispatch of the aggregate template family
// ---------------------------------------------------------------------------
struct AggArgs;
template <int VW>
void launch_expr_cm(int xm, int cm, dim3 grid, dim3 blk, hipStream_t s, const AggArgs& a);

struct AggArgs {
  const int64_t* indptr; const int32_t* indices; int64_t n_rows;
  PlanView plan; int use_plan; int64_t chunk; int x_is_row;
  const void* x; int64_t ldx; int F;
  const float* w; int64_t ldw; int gsz;
  const float* row_scale; float* y; int64_t ldy; int accumulate; float* partial;
  const void* xs; int64_t ldxs; const float* self_scale;  // gta_aggregate_self's term (xs: x's dtype)
  int y_bf16;                                            // y stored as bf16 (gta_aggregate_self, y_dtype)
  ExprArgs ex;                                           // gta_aggregate_expr's operands (XM_EX*)
};

// One wave per row, kWavesPerBlock rows per block (rows: or a bound on the work items of a plan)
inline dim3 row_grid(int64_t n_rows) { return dim3(static_cast<unsigned>((n_rows + kWavesPerBlock - 1) / kWavesPerBlock)); }

template <int LPE, int VW, int NV, int XM, int WM, typename TX, int URX = 0>
void launch_agg(const AggArgs& a, int64_t n_items_bound, hipStream_t s) {
  k_aggregate<LPE, VW, NV, XM, WM, TX, URX><<<row_grid(n_items_bound), dim3(kBlock), 0, s>>>(
      a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.chunk, a.x_is_row, static_cast<const TX*>(a.x), a.ldx, a.F,
      a.w, a.ldw, a.gsz, a.row_scale, a.y, a.ldy, a.accumulate, a.partial, static_cast<const TX*>(a.xs), a.ldxs,
      a.self_scale, a.y_bf16, a.ex);
}

template <int VW, int XM, int CM>
void launch_expr_one(dim3 grid, dim3 blk, hipStream_t s, const AggArgs& a) {
  k_agg_expr<VW, XM, CM><<<grid, blk, 0, s>>>(a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.chunk, a.ex, a.y,
                                              a.ldy, a.partial, a.F);
}

template <int VW, int XM, int... CMs>
void launch_expr_masks(int cm, dim3 grid, dim3 blk, hipStream_t s, const AggArgs& a, std::integer_sequence<int, CMs...>) {
  ((cm == CMs ? (launch_expr_one<VW, XM, CMs>(grid, blk, s, a), 0) : 0), ...);
}

template <int VW>
void launch_expr_cm(int xm, int cm, dim3 grid, dim3 blk, hipStream_t s, const AggArgs& a) {
  if (xm == XM_EX1) launch_expr_masks<VW, XM_EX1>(cm, grid, blk, s, a, std::make_integer_sequence<int, 4>{});
  else if (xm == XM_EX2) launch_expr_masks<VW, XM_EX2>(cm, grid, blk, s, a, std::make_integer_sequence<int, 8>{});
  else launch_expr_masks<VW, XM_EX3>(cm, grid, blk, s, a, std::make_integer_sequence<int, 16>{});
}

// (non-temporal index/weight loads measured +3 %: plain loads throughout)
// bf16 rows: indexed gathers (x_mode SRC / DST) without or with head weights only
template <int LPE, int VW, int NV, int XM>
bool dispatch_w(int wm, bool bf, const AggArgs& a, int64_t nb, hipStream_t s) {
  if (bf) {
    if constexpr (XM == XM_IDX) {
      if (wm == WM_NONE) { launch_agg<LPE, VW, NV, XM, WM_NONE, uint16_t>(a, nb, s); return true; }
      if (wm == WM_HEAD) { launch_agg<LPE, VW, NV, XM, WM_HEAD, uint16_t>(a, nb, s); return true; }
      if (wm == WM_EDGE1) { launch_agg<LPE, VW, NV, XM, WM_EDGE1, uint16_t>(a, nb, s); return true; }
    }
    return false;
  }
  switch (wm) {
    case WM_NONE: launch_agg<LPE, VW, NV, XM, WM_NONE, float>(a, nb, s); return true;
    case WM_HEAD: launch_agg<LPE, VW, NV, XM, WM_HEAD, float>(a, nb, s); return true;
    case WM_FULL: launch_agg<LPE, VW, NV, XM, WM_FULL, float>(a, nb, s); return true;
    case WM_EDGE1: launch_agg<LPE, VW, NV, XM, WM_EDGE1, float>(a, nb, s); return true;
  }
  return false;
}

// expressions (gta_aggregate_expr): fp32, unweighted; the 16-B form at every lane count, the 8-B
// form (F in [128, 256) or F % 4 == 2) at 64 lanes per edge only
template <int LPE, int VW, int NV>
bool dispatch_expr(int xm, const AggArgs& a, int64_t nb, hipStream_t s) {
  if constexpr (VW == 4 || (VW == 2 && LPE == kWave)) {
    switch (xm) {
      case XM_EX1: launch_agg<LPE, VW, NV, XM_EX1, WM_NONE, float>(a, nb, s); return true;
      case XM_EX2: launch_agg<LPE, VW, NV, XM_EX2, WM_NONE, float>(a, nb, s); return true;
      case XM_EX3: launch_agg<LPE, VW, NV, XM_EX3, WM_NONE, float>(a, nb, s); return true;
    }
  }
  return false;
}

template <int LPE, int VW, int NV>
bool dispatch_x(int xm, int wm, bool bf, const AggArgs& a, int64_t nb, hipStream_t s) {
  if (xm >= XM_EX1) return !bf && wm == WM_NONE && dispatch_expr<LPE, VW, NV>(xm, a, nb, s);
  return xm == XM_EDGE ? dispatch_w<LPE, VW, NV, XM_EDGE>(wm, bf, a, nb, s)
                       : dispatch_w<LPE, VW, NV, XM_IDX>(wm, bf, a, nb, s);
}

// the 16-B bf16 form (VW = 8): indexed gathers, unweighted or one weight per edge (GIN's sum), one
// piece per lane; ur: row loads in flight per lane per unrolled step (4: 16 rows per wave at 4 edges
// per instruction, 8: 32)
template <int LPE>
bool dispatch_bf16_vw8(int ur, int wm, const AggArgs& a, int64_t nb, hipStream_t s) {
  if (wm == WM_EDGE1) {
    if (ur == 8) launch_agg<LPE, 8, 1, XM_IDX, WM_EDGE1, uint16_t, 8>(a, nb, s);
    else launch_agg<LPE, 8, 1, XM_IDX, WM_EDGE1, uint16_t, 4>(a, nb, s);
  } else {
    if (ur == 8) launch_agg<LPE, 8, 1, XM_IDX, WM_NONE, uint16_t, 8>(a, nb, s);
    else launch_agg<LPE, 8, 1, XM_IDX, WM_NONE, uint16_t, 4>(a, nb, s);
  }
  return true;
}

// The generic forms' ladder (k_aggregate, k_reduce): fn(VW, LPE, NV) as integral constants.  64 lanes
// per edge take 1, 2 or 4 pieces per lane (the 16-B bf16 form: 1), fewer lanes one.
template <int N>
using IC = std::integral_constant<int, N>;

template <int VW, class Fn>
bool dispatch_lpe(int lpe, int nv, Fn fn) {
  switch (lpe) {
    case 64:
      if constexpr (VW < 8) {
        if (nv == 2) return fn(IC<VW>{}, IC<64>{}, IC<2>{});
        if (nv != 1) return fn(IC<VW>{}, IC<64>{}, IC<4>{});
      }
      return fn(IC<VW>{}, IC<64>{}, IC<1>{});
    case 32: return fn(IC<VW>{}, IC<32>{}, IC<1>{});
    case 16: return fn(IC<VW>{}, IC<16>{}, IC<1>{});
    case 8: return fn(IC<VW>{}, IC<8>{}, IC<1>{});
    default: return fn(IC<VW>{}, IC<4>{}, IC<1>{});
  }
}

template <class Fn>
bool dispatch_vw(int vw, int lpe, int nv, Fn fn) {  // VW 4, 2 or 1
  return vw == 4 ? dispatch_lpe<4>(lpe, nv, fn) : (vw == 2 ? dispatch_lpe<2>(lpe, nv, fn) : dispatch_lpe<1>(lpe, nv, fn));
}

// Tuning knobs (gta_debug_set / gta_tuning_*): per calling THREAD, or per stream when a knob set
// is attached to it, so a knob set by one caller never changes another's calls.  The defaults are
// the measured choices.  Every knob selects between forms that the defaults reach on
// some shape (the bitwise form-equality tests use them) or splits a launch for per-kernel timing;
// variants measured slower and reachable only by a knob were removed in round 3 (their A/B numbers
// stay in DESIGN.md).
struct Tuning {
  int force_lpe = 0;       // k_aggregate lanes per edge (0 = automatic; 32 = float4 lanes at F = 128)
  int force_vw = 0;        // k_aggregate floats per lane (0 = widest aligned)
  int agg_lean = 1;        // k_agg_lean for F = 64*VW SpMM shapes (0: k_aggregate, the form of other shapes)
  int seg_lean = 1;        // k_agg_h32 (32-bit row offsets, unmasked full steps, DPP weights) for F = 128
  int seg_lean_w1 = 1;     // k_agg_h32 with one weight per edge (H = 1: GCN, GraphSAGE-mean) for F = 128
  int seg_pf = 0;          // k_agg_h32pf: alpha / index lines pre-fetched into L2 by scalar loads (1: 64-B granules,
                           // 1 step ahead; 2: 128 B, 1 step; 3: 64 B, 2 steps; 4: 128 B, 2 steps; 5: as 1, held to
                           // 8 waves per SIMD; 0: off)
  int seg_alpha1 = 1;      // k_agg_h32 with 8 heads: one 8-B weight load per lane and step (A1) instead of two 4-B
  int seg_grid = 1;        // the A1 form with its steps on the aligned 8-edge grid (ldw == 8, w and indices 128-B
                           // aligned): every weight load two whole lines, every index load one
  int agg_bf16_vw8 = 4;    // k_aggregate over bf16 rows in 16-B pieces (VW = 8) instead of 8-B pieces:
                           // 0 off, 4 / 8 = row loads in flight per lane and step (1 = 4)
  int agg_w1 = 1;          // k_aggregate with one weight per edge: 64 per load, broadcast (WM_EDGE1); 0 = WM_HEAD
  int expr_lean = 1;       // k_agg_expr for gta_aggregate_expr at F = 128 / 256 (0: k_aggregate's XM_EX* form)
  int seg_class_major = 1; // blocked plan build: items numbered degree class by degree class (0: fine-block-major
                           // over all rows, the order before the classes; same results bit for bit)
  int seg_fine_pct = 100;  // default blocked plan (caller names neither item_edges nor row_edges): fine blocks =
                           // min(63, round(blocks * pct / 100)) ...
  int seg_row_edges = 10;  // ... and its row_edges (light rows merge blocks toward this many edges per item) ...
                           // (100, 10): the best point of profiles/blocked_classes/sweep_*.jsonl, DESIGN.md 3.1
  int seg_fine_min = 16;   // ... for requests of at least this many blocks; smaller ones are built as asked
  int seg_item_edges = 0;  // the default plan's item_edges (0 = the front end's default, 256)
  int seg_phase = 0;       // blocked aggregate: 0 = items + reduce, 1 = items only, 2 = reduce only (bench timing)
  int att_lean = 1;        // k_att_h32 for the fused GAT aggregate at F = 128, 8 heads (0: the generic half-wave form)
  int att_direct = 1;      // k_att_h32: a row's only item writes y itself (1: at B <= 2, 2: always, 0: never)
  int apply_node_vec = 1;  // k_apply_node4 (float4, 32-bit index math) for the common apply_node shapes
  int apply_edge_form = 1; // 1: row-sweep K3 kernels (cols / pack); 0: the generic per-element kernel
  int esm_lane = 1;        // edge-per-lane edge-softmax when H in {4,8,16} and rows are 16-B aligned
  int mm_ring = 1;         // fp32 UPDATE on k_mm_ring (LDS-DMA ring) instead of k_mm_rows
  int mm_ring_fr = 0;      // k_mm_ring A fragments per wave: 2 = 128-row groups, 1 = 64-row groups, 0 = auto
  int mm_prefetch = 1;     // k_mm_rows A prefetch: 1 auto, 2 always, 0 never
  int64_t mm_split = -1;   // UPDATE K slices: -1 auto, 0 = never split, n = n slices
  int mm_wave = 1;         // fp32 UPDATE on k_mm_wave (one wave per block, operands in registers): 0 never, 1 auto, 2 always
  int mm_wave_fr = 0;      // k_mm_wave row fragments per wave: 2, 3 or 4 (0 = auto: the best CU balance)
};

Tuning& thread_tuning() {  // gta_debug_set / gta_debug_get: the calling thread's knobs
  thread_local Tuning t;
  return t;
}

// Knob sets attached to streams (gta_tuning_attach): a call on an attached stream reads a copy
// of that set, taken at the call's entry, from whichever thread it comes; other calls read the
// calling thread's knobs.  g_attached_n keeps the common case (nothing attached) lock-free.
std::mutex g_attach_mu;
std::map<void*, Tuning> g_attached;
std::atomic<int> g_attached_n{0};
thread_local const Tuning* t_call = nullptr;

struct CallTuning {
  const Tuning* prev = t_call;
  Tuning snap;
  explicit CallTuning(void* stream) {
    if (g_attached_n.load(std::memory_order_acquire) == 0) return;
    std::lock_guard<std::mutex> lk(g_attach_mu);
    auto it = g_attached.find(stream);
    if (it == g_attached.end()) return;
    snap = it->second;
    t_call = &snap;
  }
  ~CallTuning() { t_call = prev; }
  CallTuning(const CallTuning&) = delete;
  CallTuning& operator=(const CallTuning&) = delete;
};

const Tuning& tuning() { return t_call ? *t_call : thread_tuning(); }

// Tuning hooks (gta.h): the calling thread's knobs, by name
struct Knob {
  const char* key;
  int Tuning::*i32;
  int64_t Tuning::*i64;
};

const Knob* find_knob(const char* key) {
  static const Knob knobs[] = {
      {"agg_lpe", &Tuning::force_lpe, nullptr},
      {"agg_vw", &Tuning::force_vw, nullptr},
      {"agg_lean", &Tuning::agg_lean, nullptr},
      {"seg_lean", &Tuning::seg_lean, nullptr},
      {"seg_lean_w1", &Tuning::seg_lean_w1, nullptr},
      {"seg_alpha1", &Tuning::seg_alpha1, nullptr},
      {"seg_grid", &Tuning::seg_grid, nullptr},
      {"seg_pf", &Tuning::seg_pf, nullptr},
      {"agg_bf16_vw8", &Tuning::agg_bf16_vw8, nullptr},
      {"agg_w1", &Tuning::agg_w1, nullptr},
      {"expr_lean", &Tuning::expr_lean, nullptr},
      {"seg_class_major", &Tuning::seg_class_major, nullptr},
      {"seg_fine_pct", &Tuning::seg_fine_pct, nullptr},
      {"seg_row_edges", &Tuning::seg_row_edges, nullptr},
      {"seg_fine_min", &Tuning::seg_fine_min, nullptr},
      {"seg_item_edges", &Tuning::seg_item_edges, nullptr},
      {"seg_phase", &Tuning::seg_phase, nullptr},
      {"att_lean", &Tuning::att_lean, nullptr},
      {"att_direct", &Tuning::att_direct, nullptr},
      {"apply_node_vec", &Tuning::apply_node_vec, nullptr},
      {"apply_edge_form", &Tuning::apply_edge_form, nullptr},
      {"esm_lane", &Tuning::esm_lane, nullptr},
      {"mm_ring", &Tuning::mm_ring, nullptr},
      {"mm_ring_fr", &Tuning::mm_ring_fr, nullptr},
      {"mm_prefetch", &Tuning::mm_prefetch, nullptr},
      {"mm_split", nullptr, &Tuning::mm_split},
      {"mm_wave", &Tuning::mm_wave, nullptr},
      {"mm_wave_fr", &Tuning::mm_wave_fr, nullptr},
  };
  const std::string k(key ? key : "");
  for (const Knob& kb : knobs)
    if (k == kb.key) return &kb;
  return nullptr;
}

}  // namespace

// ===========================================================================
// extern "C" ABI
// ===========================================================================
extern "C" {

int gta_abi_version(void) { return GTA_ABI_VERSION; }
const char* gta_last_error(void) { return g_err.c_str(); }

int gta_debug_set(const char* key, int64_t value) {
  const Knob* kb = find_knob(key);
  if (!kb) return fail(GTA_ERR_ARG, std::string("gta_debug_set: unknown key ") + (key ? key : ""));
  if (kb->i32) thread_tuning().*(kb->i32) = static_cast<int>(value);
  else thread_tuning().*(kb->i64) = value;
  return GTA_OK;
}

int gta_debug_get(const char* key, int64_t* value) {
  const Knob* kb = find_knob(key);
  if (!kb || !value) return fail(GTA_ERR_ARG, std::string("gta_debug_get: unknown key ") + (key ? key : ""));
  *value = kb->i32 ? static_cast<int64_t>(thread_tuning().*(kb->i32)) : thread_tuning().*(kb->i64);
  return GTA_OK;
}

}  // extern "C"

struct gta_tuning {  // a knob set (gta.h): the defaults until gta_tuning_set
  Tuning t;
};

extern "C" {

gta_tuning* gta_tuning_create(void) { return new (std::nothrow) gta_tuning{}; }

void gta_tuning_destroy(gta_tuning* h) { delete h; }

int gta_tuning_set(gta_tuning* h, const char* key, int64_t value) {
  const Knob* kb = find_knob(key);
  if (!h || !kb) return fail(GTA_ERR_ARG, std::string("gta_tuning_set: bad handle or unknown key ") + (key ? key : ""));
  if (kb->i32) h->t.*(kb->i32) = static_cast<int>(value);
  else h->t.*(kb->i64) = value;
  return GTA_OK;
}

int gta_tuning_get(const gta_tuning* h, const char* key, int64_t* value) {
  const Knob* kb = find_knob(key);
  if (!h || !kb || !value) return fail(GTA_ERR_ARG, std::string("gta_tuning_get: bad arguments ") + (key ? key : ""));
  *value = kb->i32 ? static_cast<int64_t>(h->t.*(kb->i32)) : h->t.*(kb->i64);
  return GTA_OK;
}

int gta_tuning_attach(void* stream, const gta_tuning* h) {
  std::lock_guard<std::mutex> lk(g_attach_mu);
  if (h) g_attached[stream] = h->t;
  else g_attached.erase(stream);
  g_attached_n.store(static_cast<int>(g_attached.size()), std::memory_order_release);
  return GTA_OK;
}

int64_t gta_aggregate_plan_bytes(int64_t n_rows, int64_t nnz, int64_t chunk) {
  if (n_rows < 0 || nnz < 0 || chunk <= 0) return fail(GTA_ERR_ARG, "plan_bytes: bad sizes");
  return plan_bytes_for(n_rows, max_items_for(n_rows, nnz, chunk));
}

int64_t gta_aggregate_workspace_bytes(int64_t n_rows, int64_t nnz, int64_t chunk, int64_t F) {
  if (n_rows < 0 || nnz < 0 || chunk <= 0 || F <= 0) return fail(GTA_ERR_ARG, "workspace_bytes: bad sizes");
  return max_items_for(n_rows, nnz, chunk) * F * static_cast<int64_t>(sizeof(float));
}

int gta_aggregate_plan_build(const int64_t* indptr, int64_t n_rows, int64_t nnz, int64_t chunk, void* plan,
                             int64_t plan_bytes, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (!indptr || !plan || n_rows <= 0 || chunk <= 0 || (chunk % kWave) != 0)
    return fail(GTA_ERR_ARG, "plan_build: need indptr, plan, n_rows > 0 and chunk a positive multiple of 64");
  const int64_t mi = max_items_for(n_rows, nnz, chunk);
  if (plan_bytes < plan_bytes_for(n_rows, mi)) return fail(GTA_ERR_ARG, "plan_build: plan buffer too small");
  if (n_rows > INT32_MAX || mi > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "plan_build: > 2^31 rows/items");
  PlanView v = plan_view(plan, n_rows, mi);
  hipStream_t s = S(stream);
  k_plan_scan<<<1, 1024, 0, s>>>(indptr, n_rows, chunk, v.offs, v.hdr);
  GTA_LAUNCHED("k_plan_scan");
  k_plan_fill<<<dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, s>>>(indptr, n_rows, chunk, v);
  GTA_LAUNCHED("k_plan_fill");
  return GTA_OK;
}

}  // extern "C"
namespace {
// The generic gather forms' shape for rows of F elements (aggregate_impl, reduce_impl).  vw: the
// widest vector at which every access stays aligned (ok_vw, the caller's layout test); one edge
// per wave instruction (LPE = 64, wave-uniform row base) whenever the row fills 64 lanes at
// >= 8 B/lane: measured 3 % faster than two edges per instruction at float4 for F = 128
// (profiles/r01_agg_sweep_1.json).  lpe_knob: the caller honours agg_lpe at F = 128.
// vw8: bf16 rows gathered in 16-B pieces (8 elements per lane, the last lane's piece clamped
// inside the row) where the caller's layout admits them (vw8_ok): half the gather instructions of
// 8-B pieces for the same rows (GIN products' 200-B rows: 13 lanes, 4 edges per wave instruction).
struct GatherShape {
  int vw, lpe, nv;
  bool vw8;
};

template <class OkVw>
GatherShape gather_shape(int64_t F, bool bf, OkVw ok_vw, bool lpe_knob, bool vw8_ok) {
  const Tuning& t = tuning();
  GatherShape g{ok_vw(4) ? 4 : (ok_vw(2) ? 2 : 1), 4, 1, false};
  if (t.force_vw && t.force_vw <= g.vw && ok_vw(t.force_vw)) g.vw = t.force_vw;
  if (!bf && g.vw == 4 && F < 4 * kWave && F >= 2 * kWave && ok_vw(2)) g.vw = 2;
  g.vw8 = bf && t.agg_bf16_vw8 && F % 4 == 0 && F >= 8 && F <= 512 && vw8_ok;
  if (g.vw8) g.vw = 8;  // at most 64 lanes, one piece each
  const int64_t lanes = (F + g.vw - 1) / g.vw;
  if (lanes >= kWave) {
    g.lpe = kWave;
    g.nv = lanes >= 4 * kWave ? 4 : (lanes > kWave ? 2 : 1);
  } else {
    while (g.lpe < lanes) g.lpe <<= 1;
  }
  if (lpe_knob && !bf && t.force_lpe == 32 && F == 128 && ok_vw(4)) g = {4, 32, 1, false};
  if (lpe_knob && !bf && t.force_lpe == 64 && F == 128 && ok_vw(2)) g = {2, 64, 1, false};
  return g;
}

// the arguments every per-row gather kernel takes; returns the bound on its work items (the rows,
// or what the plan can hold), or fail()'s code
int64_t gather_args(AggArgs& a, const char* who, const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                    int64_t nnz, int x_mode, const void* x, int64_t ldx, int64_t F, float* y, int64_t ldy,
                    const void* plan, int64_t plan_chunk, void* workspace) {
  a.indptr = indptr; a.indices = indices; a.n_rows = n_rows;
  a.use_plan = plan != nullptr; a.chunk = plan_chunk; a.x_is_row = (x_mode == GTA_IDX_DST);
  a.x = x; a.ldx = ldx; a.F = static_cast<int>(F); a.y = y; a.ldy = ldy;
  a.partial = static_cast<float*>(workspace);
  if (!plan) return n_rows;
  if (plan_chunk <= 0 || !workspace) return fail(GTA_ERR_ARG, std::string(who) + ": plan needs chunk and workspace");
  const int64_t bound = max_items_for(n_rows, nnz, plan_chunk);
  a.plan = plan_view(const_cast<void*>(plan), n_rows, bound);
  return bound;
}

// the combine launch over a plan's split rows (at most one per chunk of edges), if there can be any
template <class Launch>
bool launch_combine(int64_t nnz, int64_t plan_chunk, Launch launch) {
  const int64_t sb = (nnz + plan_chunk - 1) / plan_chunk;  // >= number of split rows
  if (sb > 0) launch(row_grid(sb));
  return sb > 0;
}

int aggregate_impl(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
                   const void* x, int64_t ldx, int64_t F, int x_dtype, const float* w, int64_t ldw, int64_t heads,
                   const float* row_scale, float* y, int64_t ldy, int accumulate, const void* plan,
                   int64_t plan_chunk, void* workspace, void* stream, const void* xs, int64_t ldxs,
                   const float* self_scale, int y_bf16 = 0, const ExprArgs* ex = nullptr, int ex_mode = 0) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || nnz < 0 || F <= 0) return fail(GTA_ERR_ARG, "aggregate: bad sizes");
  ExprArgs exa{};
  if (ex) {  // gta_aggregate_expr: x_mode / x / w unused; every edge reads its source index
    exa = *ex;
    x_mode = GTA_IDX_EDGE;
    x = exa.p[0];
    w = nullptr;
    if (nnz > 0 && !indices) return fail(GTA_ERR_ARG, "aggregate_expr: indices is NULL");
    if (nnz == 0) {  // no edge is read; the per-item operand loads read y's first row instead
      for (int l = 0; l < 4; ++l) { exa.p[l] = y; exa.ld[l] = 0; }
      exa.code &= ~0xff;  // every mode GTA_IDX_EDGE
    }
  }
  if (y_bf16 && (accumulate || ldy < F)) return fail(GTA_ERR_ARG, "aggregate: a bf16 y takes no accumulate; ldy >= F");
  if (xs && (accumulate || ldxs < F)) return fail(GTA_ERR_ARG, "aggregate_self: no accumulate; ld_self >= F");
  if (x_mode != GTA_IDX_EDGE && x_mode != GTA_IDX_SRC && x_mode != GTA_IDX_DST)
    return fail(GTA_ERR_ARG, "aggregate: bad x_mode");
  if (x_dtype != GTA_F32 && x_dtype != GTA_BF16) return fail(GTA_ERR_ARG, "aggregate: x_dtype must be F32 or BF16");
  const bool bf = x_dtype == GTA_BF16;
  const int xe = bf ? 2 : 4;  // bytes per x element
  if (bf && (x_mode == GTA_IDX_EDGE || (w && heads == F)))
    return fail(GTA_ERR_UNSUPPORTED, "aggregate: bf16 rows are gathered by index (SRC / DST) with head weights or none");
  if (F > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "aggregate: F too large");
  if (n_rows == 0) return GTA_OK;
  // with no edges, indices / edge operands are never read (may be NULL); every row gets 0
  if (!indptr || !y || (nnz > 0 && !x)) return fail(GTA_ERR_ARG, "aggregate: bad arguments");
  if (x_mode == GTA_IDX_SRC && !indices && nnz > 0) return fail(GTA_ERR_ARG, "aggregate: x_mode SRC needs indices");
  if (nnz == 0) {
    x = y;  // any valid address: no row has an edge to read
    w = nullptr;
  }
  int wm = WM_NONE, gsz = 1;
  if (w) {
    if (heads <= 0 || F % heads != 0) return fail(GTA_ERR_ARG, "aggregate: heads must divide F");
    wm = (heads == F) ? WM_FULL : ((heads == 1 && tuning().agg_w1) ? WM_EDGE1 : WM_HEAD);
    gsz = static_cast<int>(F / heads);
  }
  const int xm = ex ? ex_mode : ((x_mode == GTA_IDX_EDGE) ? XM_EDGE : XM_IDX);
  // widest vector that keeps every access aligned (an expression: the width its unfused gather
  // of a fresh [E, F] edge tensor takes -- its operands must allow it, checked below)
  auto ok_vw = [&](int vw) {
    if (ex) return F % vw == 0 && ldy % vw == 0 && aligned(y, 4 * vw);
    if (F % vw || ldx % vw || ldy % vw || !aligned(x, xe * vw) || !aligned(y, (y_bf16 ? 2 : 4) * vw)) return false;
    if (xs && (ldxs % vw || !aligned(xs, xe * vw))) return false;
    if (wm == WM_HEAD && gsz % vw) return false;
    if (wm == WM_FULL && (ldw % vw || !aligned(w, 4 * vw))) return false;
    return true;
  };
  // the 16-B bf16 form: unweighted or one weight per edge, indexed, xs and y (fp32 or bf16) aligned to it
  const bool vw8_ok = (wm == WM_NONE || wm == WM_EDGE1) && xm == XM_IDX && ldx % 4 == 0 && aligned(x, 8) &&
                      (!xs || (ldxs % 4 == 0 && aligned(xs, 8))) && ldy % 4 == 0 && aligned(y, y_bf16 ? 8 : 16);
  const GatherShape g = gather_shape(F, bf, ok_vw, /*lpe_knob=*/true, vw8_ok);
  const int vw = g.vw, lpe = g.lpe, nv = g.nv;

  if (ex) {
    const int nl = ex_mode == XM_EX1 ? (ex_bin(exa.code, 0) == GTA_BIN_NONE ? 1 : 2) : (ex_mode == XM_EX2 ? 3 : 4);
    for (int l = 0; l < nl; ++l)
      if (exa.ld[l] % vw || !aligned(exa.p[l], 4 * vw))
        return fail(GTA_ERR_UNSUPPORTED, "aggregate_expr: an operand's rows are not aligned to the gather's vector width");
  }
  AggArgs a{};
  const int64_t bound = gather_args(a, "aggregate", indptr, indices, n_rows, nnz, x_mode, x, ldx, F, y, ldy, plan,
                                    plan_chunk, workspace);
  if (bound < 0) return static_cast<int>(bound);
  a.ex = exa;
  a.w = w; a.ldw = ldw; a.gsz = gsz; a.row_scale = row_scale; a.accumulate = accumulate;
  a.xs = xs; a.ldxs = ldxs; a.self_scale = self_scale; a.y_bf16 = y_bf16;
  hipStream_t s = S(stream);
  bool ok = false;
  // lean path: one edge per instruction exactly filling the wave, SpMM form
  int gl = (wm == WM_HEAD) ? gsz / vw : 0;
  const bool lean_shape = !bf && !y_bf16 && tuning().agg_lean && lpe == kWave && nv == 1 && F == kWave * vw && xm == XM_IDX &&
                          !a.x_is_row && wm != WM_FULL && wm != WM_EDGE1 && (wm == WM_NONE || gl == 4 || gl == 8 || gl == 16);
  if (lean_shape) {
    const dim3 grid = row_grid(bound), blk(kBlock);
#define GTA_LEAN(VW_, GL_)                                                                                   \
  k_agg_lean<VW_, GL_><<<grid, blk, 0, s>>>(a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.chunk, \
                                            static_cast<const float*>(a.x), a.ldx, a.F, a.w, a.ldw, a.row_scale, \
                                            a.y, a.ldy, a.accumulate, a.partial, static_cast<const float*>(a.xs), \
                                            a.ldxs, a.self_scale)
    if (vw == 2) {
      if (gl == 0) GTA_LEAN(2, 0); else if (gl == 4) GTA_LEAN(2, 4); else if (gl == 8) GTA_LEAN(2, 8); else GTA_LEAN(2, 16);
    } else if (vw == 4) {
      if (gl == 0) GTA_LEAN(4, 0); else if (gl == 4) GTA_LEAN(4, 4); else if (gl == 8) GTA_LEAN(4, 8); else GTA_LEAN(4, 16);
    } else {
      if (gl == 0) GTA_LEAN(1, 0); else if (gl == 4) GTA_LEAN(1, 4); else if (gl == 8) GTA_LEAN(1, 8); else GTA_LEAN(1, 16);
    }
#undef GTA_LEAN
    ok = true;
  }
  // k_agg_expr masks no column: only rows that exactly fill the wave (F = 128 at VW 2, 256 at VW 4).
  // lpe == kWave alone also holds for 33..63 lanes (F = 66..126 at VW 2, 132..252 at VW 4), whose
  // idle lanes would load and store past column F: those widths take k_aggregate's XM_EX* form
  if (!ok && ex && tuning().expr_lean && lpe == kWave && nv == 1 && (vw == 2 || vw == 4) && F == kWave * vw) {
    const dim3 grid = row_grid(bound), blk(kBlock);
#define GTA_EXPR(VW_, XM_)                                                                                   \
  k_agg_expr<VW_, XM_><<<grid, blk, 0, s>>>(a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.chunk, a.ex, a.y, \
                                          a.ldy, a.partial, a.F)
    if (vw == 2) {  // F = 128 (the genGraphOP layer-1 width): the row-constant operands as a template mask
      int cm = 0;
      const int nl = xm == XM_EX1 ? 2 : (xm == XM_EX2 ? 3 : 4);
      for (int l = 0; l < nl; ++l) {
        const int md = (a.ex.code >> (2 * l)) & 3;  // ex_mode() (a parameter here shadows its name)
        if (md == GTA_IDX_DST || (md == GTA_IDX_EDGE && a.ex.ld[l] == 0)) cm |= 1 << l;
      }
      launch_expr_cm<2>(xm, cm, grid, blk, s, a);
    } else {
      if (xm == XM_EX1) GTA_EXPR(4, XM_EX1); else if (xm == XM_EX2) GTA_EXPR(4, XM_EX2); else GTA_EXPR(4, XM_EX3);
    }
#undef GTA_EXPR
    ok = true;
  }
  if (!ok && g.vw8) {
    ok = dispatch_lpe<8>(lpe, 1, [&](auto, auto L, auto) {
      return dispatch_bf16_vw8<L()>(tuning().agg_bf16_vw8, wm, a, bound, s);
    });
  } else if (!ok) {
    ok = dispatch_vw(vw, lpe, nv, [&](auto V, auto L, auto N) { return dispatch_x<L(), V(), N()>(xm, wm, bf, a, bound, s); });
  }
  if (!ok) return fail(GTA_ERR_UNSUPPORTED, "aggregate: no kernel variant");
  GTA_LAUNCHED("k_aggregate");
  const bool combined = plan && launch_combine(nnz, plan_chunk, [&](dim3 grid) {
    k_aggregate_combine<<<grid, dim3(kBlock), 0, s>>>(a.plan, a.F, row_scale, y, ldy, accumulate, a.partial, xs, ldxs,
                                                      bf ? 1 : 0, self_scale, y_bf16);
  });
  if (combined) GTA_LAUNCHED("k_aggregate_combine");
  return GTA_OK;
}

// ---- host side of the row reducers (gta_reduce MAX / MIN here; gta_reduce_multi after with_bools) ----

// The checks both entry points make, in two parts: reduce_multi_impl checks its output arrays between
// them.  First the sizes, x_mode, x_dtype and what the kernels cannot take; 0 or fail()'s code
int reduce_check_call(const std::string& who, int64_t n_rows, int64_t nnz, int x_mode, int64_t F, int x_dtype) {
  if (n_rows < 0 || nnz < 0 || F <= 0) return fail(GTA_ERR_ARG, who + ": bad sizes");
  if (x_mode != GTA_IDX_EDGE && x_mode != GTA_IDX_SRC && x_mode != GTA_IDX_DST)
    return fail(GTA_ERR_ARG, who + ": bad x_mode");
  if (x_dtype != GTA_F32 && x_dtype != GTA_BF16) return fail(GTA_ERR_ARG, who + ": x_dtype must be F32 or BF16");
  if (x_dtype == GTA_BF16 && x_mode == GTA_IDX_EDGE)
    return fail(GTA_ERR_UNSUPPORTED, who + ": bf16 rows are gathered by index (SRC / DST)");
  if (F > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, who + ": F too large");
  return GTA_OK;
}

// Then, with rows to write, the pointers and row strides (y: the output, or the first of several).
// With no edges, x and indices are never read (may be NULL) and every row gets 0: x becomes y, any
// valid address
int reduce_check_operand(const std::string& who, const int64_t* indptr, const int32_t* indices, int64_t nnz, int x_mode,
                         const void*& x, int64_t& ldx, int64_t F, const float* y, int64_t ldy) {
  if (!indptr || !y || (nnz > 0 && !x) || ldy < F || (nnz > 0 && ldx < F)) return fail(GTA_ERR_ARG, who + ": bad arguments");
  if (x_mode == GTA_IDX_SRC && !indices && nnz > 0) return fail(GTA_ERR_ARG, who + ": x_mode SRC needs indices");
  if (nnz == 0) { x = y; ldx = ldy; }
  return GTA_OK;
}

// The reducers' ladder over a GatherShape: fn(LPE, VW, NV, XM as integral constants, TX{}).  bf16 rows
// are gathered by index only (false: no such kernel), fp32 rows by edge or by index; the 16-B bf16
// form (g.vw8) exists for indexed bf16 rows alone
template <class Fn>
bool dispatch_xm(int xm, bool bf, Fn fn) {
  if (bf && xm != XM_IDX) return false;
  if (bf) fn(IC<XM_IDX>{}, uint16_t{});
  else if (xm == XM_EDGE) fn(IC<XM_EDGE>{}, float{});
  else fn(IC<XM_IDX>{}, float{});
  return true;
}

template <class Fn>
bool dispatch_gather(const GatherShape& g, int xm, bool bf, Fn fn) {
  if (g.vw8) {
    return dispatch_lpe<8>(g.lpe, 1, [&](auto V, auto L, auto N) {
      fn(L, V, N, IC<XM_IDX>{}, uint16_t{});
      return true;
    });
  }
  return dispatch_vw(g.vw, g.lpe, g.nv, [&](auto V, auto L, auto N) {
    return dispatch_xm(xm, bf, [&](auto X, auto tx) { fn(L, V, N, X, tx); });
  });
}

template <int LPE, int VW, int NV, int XM, typename TX>
void launch_red(const AggArgs& a, uint32_t sbit, int64_t n_items_bound, hipStream_t s) {
  k_reduce<LPE, VW, NV, XM, TX><<<row_grid(n_items_bound), dim3(kBlock), 0, s>>>(
      a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.x_is_row, static_cast<const TX*>(a.x), a.ldx, a.F, sbit,
      a.y, a.ldy, a.partial);
}

// gta_reduce MAX / MIN: aggregate_impl's choice of LPE / VW / NV
int reduce_impl(int red, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
                const void* x, int64_t ldx, int64_t F, int x_dtype, float* y, int64_t ldy, const void* plan,
                int64_t plan_chunk, void* workspace, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (const int rc = reduce_check_call("reduce", n_rows, nnz, x_mode, F, x_dtype)) return rc;
  if (n_rows == 0) return GTA_OK;
  if (const int rc = reduce_check_operand("reduce", indptr, indices, nnz, x_mode, x, ldx, F, y, ldy)) return rc;
  const bool bf = x_dtype == GTA_BF16;
  const int xe = bf ? 2 : 4;  // bytes per x element
  const int xm = (x_mode == GTA_IDX_EDGE) ? XM_EDGE : XM_IDX;
  auto ok_vw = [&](int vw) {
    return !(F % vw || ldx % vw || ldy % vw || !aligned(x, xe * vw) || !aligned(y, 4 * vw));
  };
  // the 16-B bf16 form: only with edges to read (x is y's fp32 rows otherwise) and no agg_vw knob
  const bool vw8_ok = nnz > 0 && !tuning().force_vw && ldx % 4 == 0 && aligned(x, 8) && ldy % 4 == 0 && aligned(y, 16);
  const GatherShape g = gather_shape(F, bf, ok_vw, /*lpe_knob=*/false, vw8_ok);
  AggArgs a{};
  const int64_t bound = gather_args(a, "reduce", indptr, indices, n_rows, nnz, x_mode, x, ldx, F, y, ldy, plan,
                                    plan_chunk, workspace);
  if (bound < 0) return static_cast<int>(bound);
  const uint32_t sbit = red == GTA_RED_MIN ? 0x80000000u : 0u;
  hipStream_t s = S(stream);
  const bool ok = dispatch_gather(g, xm, bf, [&](auto L, auto V, auto N, auto X, auto tx) {
    launch_red<L(), V(), N(), X(), decltype(tx)>(a, sbit, bound, s);
  });
  if (!ok) return fail(GTA_ERR_UNSUPPORTED, "reduce: no kernel variant");
  GTA_LAUNCHED("k_reduce");
  const bool combined = plan && launch_combine(nnz, plan_chunk, [&](dim3 grid) {
    k_reduce_combine<<<grid, dim3(kBlock), 0, s>>>(a.plan, a.F, sbit, y, ldy, a.partial);
  });
  if (combined) GTA_LAUNCHED("k_reduce_combine");
  return GTA_OK;
}

// ---- host side of the column-blocked entry points (aggregate, reduce, GAT aggregate) ----

// What the three families read from a blocked plan and its workspace: built after the family's own
// argument checks, it touches no memory (pointer arithmetic on the plan's layout and the grids).
struct BlockedCall {
  BlockedView v;
  RowItems ri;
  float* slabs;        // per-item slab rows (the workspace)
  const int64_t* nit;  // the plan's n_items, read by the kernels
  const SegItem* its;
  int64_t items;       // grid bound (blocked_max_items); the kernels stop at *nit
  dim3 g2, g2h, g4;    // item grids: one, two (half-wave) and four (quarter-wave) items per wave
  dim3 g3;             // the ordered reduce: one wave per row
  dim3 blk{kBlock};
  hipStream_t s;
  BlockedCall(const void* plan, int64_t n_rows, int64_t nnz, int64_t blocks, int64_t item_edges, void* workspace,
              void* stream)
      : items(blocked_max_items(n_rows, nnz, static_cast<int>(blocks), item_edges)), s(S(stream)) {
    v = blocked_view(const_cast<void*>(plan), n_rows, static_cast<int>(blocks), items);
    ri = RowItems{v.row_ptr, v.row_items};
    slabs = static_cast<float*>(workspace);
    nit = &v.hdr[4];
    its = v.items;
    auto grid = [](int64_t n, int per_block) { return dim3(static_cast<unsigned>((n + per_block - 1) / per_block)); };
    g2 = grid(items, kWavesPerBlock);
    g2h = grid(items, 2 * kWavesPerBlock);
    g4 = grid(items, 4 * kWavesPerBlock);
    g3 = grid(n_rows, kWavesPerBlock);
  }
};

// The lean kernels' 32-bit row addressing (lean_at): row ids fit the 24-bit multiply and the table
// spans < 2^32 bytes, in the table's own element size
inline bool lean32_ok(int64_t n_cols, int64_t ld, unsigned elem_bytes) {
  return n_cols < (1 << 24) && static_cast<uint64_t>(n_cols) * static_cast<uint64_t>(ld) * elem_bytes < (1ull << 32);
}

// Run-time bools as compile-time constants for a generic lambda, next to dispatch_lpe's IC:
// with_bools(fn, a, b) calls fn(BC<a>{}, BC<b>{}), so a ladder over template flags is written once.
template <bool V>
using BC = std::integral_constant<bool, V>;

template <class Fn>
void with_bools(Fn fn) { fn(); }
template <class Fn, class... Rest>
void with_bools(Fn fn, bool b, Rest... rest) {
  if (b) with_bools([&](auto... cs) { fn(BC<true>{}, cs...); }, rest...);
  else with_bools([&](auto... cs) { fn(BC<false>{}, cs...); }, rest...);
}

// The vector-width ladder fn(IC<VW>), VW in 1, 2, 4: k_seg_reduce* (F / 64), k_apply_edge_cols / _flat (vec_ok)
template <class Fn>
void dispatch_vw(int vw, Fn fn) {
  if (vw == 2) fn(IC<2>{});
  else if (vw == 4) fn(IC<4>{});
  else fn(IC<1>{});
}

// The heads ladder of the unfused softmax kernels: fn(IC<H>), heads a power of two in 1 .. 64 (check_heads)
template <class Fn>
void dispatch_heads(int64_t heads, Fn fn) {
  switch (heads) {
    case 1: return fn(IC<1>{});
    case 2: return fn(IC<2>{});
    case 4: return fn(IC<4>{});
    case 8: return fn(IC<8>{});
    case 16: return fn(IC<16>{});
    case 32: return fn(IC<32>{});
    case 64: return fn(IC<64>{});
  }
}

// May a K3 kernel move vw floats per lane?  out and each full-width operand (g == 1) vw-float aligned,
// a head-broadcast operand with vw output columns in one head.  ops._flat_aligned mirrors this in Python.
bool vec_ok(int vw, const float* a, int64_t lda, int ga, const float* b, int64_t ldb, int gb, const float* out,
            int64_t ldo) {
  if (ldo % vw || !aligned(out, 4 * vw)) return false;
  if (ga == 1 ? (lda % vw || !aligned(a, 4 * vw)) : (ga % vw != 0)) return false;
  if (b && (gb == 1 ? (ldb % vw || !aligned(b, 4 * vw)) : (gb % vw != 0))) return false;
  return true;
}

// The heads / sf / leading-dimension checks of gta_edge_softmax* and gta_softmax_shift; 0 or the error code
int check_heads(const char* who, int64_t heads, int sf, bool need_exp, int64_t lda, int64_t ldb) {
  if (heads <= 0 || heads > kWave || (heads & (heads - 1)))
    return fail(GTA_ERR_UNSUPPORTED, std::string(who) + ": heads must be a power of two <= 64");
  if (need_exp && !sf_is_exp_form(sf))
    return fail(GTA_ERR_UNSUPPORTED, std::string(who) + ": sf must be EXP_LEAKY_RELU or EXP");
  if (lda < heads || ldb < heads) return fail(GTA_ERR_ARG, std::string(who) + ": leading dimension < heads");
  return GTA_OK;
}

// gta_reduce_multi: reduce_impl's path, specialised on which accumulator families the call needs
template <int LPE, int VW, int NV, int XM, typename TX>
void launch_multi(bool mom, bool ext, const AggArgs& a, const MultiOut& out, float eps, int64_t pstride,
                  int64_t n_items_bound, hipStream_t s) {
  with_bools([&](auto M, auto E) {
    if constexpr ((M() || E()) && !(M() && VW == 8))  // (the 16-B bf16 pieces carry the extrema only)
      k_reduce_multi<LPE, VW, NV, XM, M(), E(), TX><<<row_grid(n_items_bound), dim3(kBlock), 0, s>>>(
          a.indptr, a.indices, a.n_rows, a.plan, a.use_plan, a.x_is_row, static_cast<const TX*>(a.x), a.ldx, a.F, out,
          eps, a.partial, pstride);
  }, mom, ext);
}

int reduce_multi_impl(int which, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                      int x_mode, const void* x, int64_t ldx, int64_t F, int x_dtype, float* const* ys,
                      const int64_t* ldys, float std_eps, const void* plan, int64_t plan_chunk, void* workspace,
                      void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  constexpr int kAll = GTA_MR_MEAN | GTA_MR_MAX | GTA_MR_MIN | GTA_MR_VAR | GTA_MR_STD;
  if (which == 0 || (which & ~kAll)) return fail(GTA_ERR_ARG, "reduce_multi: which must be a non-empty set of GTA_MR_* bits");
  if (const int rc = reduce_check_call("reduce_multi", n_rows, nnz, x_mode, F, x_dtype)) return rc;
  if (!ys || !ldys) return fail(GTA_ERR_ARG, "reduce_multi: ys / ldys is NULL");
  MultiOut out{};
  float* y0 = nullptr;
  int64_t ldy0 = 0;
  for (int b = 0, k = 0; b < MR_N; ++b) {  // one entry per set bit, in bit order
    if (!(which >> b & 1)) continue;
    if (!ys[k] || ldys[k] < F) return fail(GTA_ERR_ARG, "reduce_multi: an output is NULL or its row stride < F");
    out.y[b] = ys[k]; out.ld[b] = ldys[k];
    if (!y0) { y0 = ys[k]; ldy0 = ldys[k]; }
    ++k;
  }
  if (n_rows == 0) return GTA_OK;
  if (const int rc = reduce_check_operand("reduce_multi", indptr, indices, nnz, x_mode, x, ldx, F, y0, ldy0)) return rc;
  const bool bf = x_dtype == GTA_BF16;
  const int xe = bf ? 2 : 4;  // bytes per x element
  const int xm = (x_mode == GTA_IDX_EDGE) ? XM_EDGE : XM_IDX;
  auto outs_ok = [&](int vw, int bytes) {  // every requested output's rows aligned to vw floats / bytes
    for (int b = 0; b < MR_N; ++b)
      if (out.y[b] && (out.ld[b] % vw || !aligned(out.y[b], bytes))) return false;
    return true;
  };
  auto ok_vw = [&](int vw) { return !(F % vw || ldx % vw || !aligned(x, xe * vw)) && outs_ok(vw, 4 * vw); };
  const bool mom = which & (GTA_MR_MEAN | GTA_MR_VAR | GTA_MR_STD), ext = which & (GTA_MR_MAX | GTA_MR_MIN);
  // The extrema do not depend on the order of the edges and take reduce_impl's shapes.  The moments'
  // sums do (each of a form's edge slots adds up its own edges): with them the shape comes from F
  // and the layout alone -- the fp32 ladder, no 16-B bf16 pieces -- so a bf16 table gives bitwise
  // the fp32 call on its widened rows
  const bool vw8_ok = !mom && nnz > 0 && !tuning().force_vw && ldx % 4 == 0 && aligned(x, 8) && outs_ok(4, 16);
  const GatherShape g = gather_shape(F, bf && !mom, ok_vw, /*lpe_knob=*/false, vw8_ok);
  AggArgs a{};
  const int64_t bound = gather_args(a, "reduce_multi", indptr, indices, n_rows, nnz, x_mode, x, ldx, F, y0, ldy0, plan,
                                    plan_chunk, workspace);
  if (bound < 0) return static_cast<int>(bound);
  const int64_t pstride = bound * F;  // one plane of partials: gta_aggregate_workspace_bytes(..., F)
  hipStream_t s = S(stream);
  const bool ok = dispatch_gather(g, xm, bf, [&](auto L, auto V, auto N, auto X, auto tx) {
    launch_multi<L(), V(), N(), X(), decltype(tx)>(mom, ext, a, out, std_eps, pstride, bound, s);
  });
  if (!ok) return fail(GTA_ERR_UNSUPPORTED, "reduce_multi: no kernel variant");
  GTA_LAUNCHED("k_reduce_multi");
  const bool combined = plan && launch_combine(nnz, plan_chunk, [&](dim3 grid) {
    with_bools([&](auto M, auto E, auto B) {
      using TX = std::conditional_t<B(), uint16_t, float>;
      if constexpr (M() || E())
        k_reduce_multi_combine<M(), E(), TX><<<grid, dim3(kBlock), 0, s>>>(
            a.plan, indptr, indices, x_mode, static_cast<const TX*>(x), ldx, a.F, out, std_eps, a.partial, pstride);
    }, mom, ext, bf);
  });
  if (combined) GTA_LAUNCHED("k_reduce_multi_combine");
  return GTA_OK;
}
}  // namespace
extern "C" {

int gta_aggregate(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
                  const void* x, int64_t ldx, int64_t F, int x_dtype, const float* w, int64_t ldw, int64_t heads,
                  const float* row_scale, float* y, int64_t ldy, int accumulate, const void* plan,
                  int64_t plan_chunk, void* workspace, void* stream) {
  return aggregate_impl(indptr, indices, n_rows, nnz, x_mode, x, ldx, F, x_dtype, w, ldw, heads, row_scale, y, ldy,
                        accumulate, plan, plan_chunk, workspace, stream, nullptr, 0, nullptr);
}

int gta_reduce(int red, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
               const void* x, int64_t ldx, int64_t F, int x_dtype, float* y, int64_t ldy, const void* plan,
               int64_t plan_chunk, void* workspace, void* stream) {
  if (red == GTA_RED_ADD) {  // the sum is gta_aggregate's: no weights, no row scale, no accumulate
    const int rc = aggregate_impl(indptr, indices, n_rows, nnz, x_mode, x, ldx, F, x_dtype, nullptr, 0, 0, nullptr, y,
                                  ldy, 0, plan, plan_chunk, workspace, stream, nullptr, 0, nullptr);
    return rc < 0 ? fail(rc, "reduce (ADD): " + g_err) : rc;
  }
  if (red != GTA_RED_MAX && red != GTA_RED_MIN)
    return fail(GTA_ERR_ARG, "reduce: red must be GTA_RED_ADD, GTA_RED_MAX or GTA_RED_MIN");
  return reduce_impl(red, indptr, indices, n_rows, nnz, x_mode, x, ldx, F, x_dtype, y, ldy, plan, plan_chunk,
                     workspace, stream);
}

int gta_reduce_multi(int which, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
                     const void* x, int64_t ldx, int64_t F, int x_dtype, float* const* ys, const int64_t* ldys,
                     float std_eps, const void* plan, int64_t plan_chunk, void* workspace, void* stream) {
  return reduce_multi_impl(which, indptr, indices, n_rows, nnz, x_mode, x, ldx, F, x_dtype, ys, ldys, std_eps, plan,
                           plan_chunk, workspace, stream);
}

int gta_aggregate_expr(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int shape,
                       const float* const* operands, const int* modes, const int64_t* lds, const int* bins,
                       const int* sfs, int swap, int64_t F, float* y, int64_t ldy, const void* plan,
                       int64_t plan_chunk, void* workspace, void* stream) {
  if (shape < 1 || shape > 3) return fail(GTA_ERR_ARG, "aggregate_expr: shape must be 1, 2 or 3");
  if (!operands || !modes || !lds || !bins || !sfs) return fail(GTA_ERR_ARG, "aggregate_expr: NULL operand arrays");
  ExprArgs ex{};
  int code = swap ? (1 << 29) : 0;
  const int n_ops = shape;
  for (int i = 0; i < n_ops; ++i) {
    const bool none_ok = shape == 1 && i == 0;
    if (bins[i] < (none_ok ? GTA_BIN_NONE : GTA_BIN_ADD) || bins[i] > GTA_BIN_SUB)
      return fail(GTA_ERR_ARG, "aggregate_expr: bad bin");
    if (sfs[i] < GTA_SF_NONE || sfs[i] > GTA_SF_RECIP) return fail(GTA_ERR_ARG, "aggregate_expr: bad sf");
    code |= (bins[i] << (8 + 3 * i)) | (sfs[i] << (17 + 4 * i));
  }
  const int nl = shape == 1 ? (bins[0] == GTA_BIN_NONE ? 1 : 2) : shape + 1;
  for (int l = 0; l < 4; ++l) {
    const int k = l < nl ? l : 0;  // unused slots repeat operand 0
    if (modes[k] != GTA_IDX_EDGE && modes[k] != GTA_IDX_SRC && modes[k] != GTA_IDX_DST)
      return fail(GTA_ERR_ARG, "aggregate_expr: bad operand mode");
    if ((lds[k] < F && !(modes[k] == GTA_IDX_EDGE && lds[k] == 0)) || (nnz > 0 && !operands[k]))
      return fail(GTA_ERR_ARG, "aggregate_expr: operand rows need ld >= F (or ld 0: a broadcast row)");
    if (lds[k] > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "aggregate_expr: operand row stride >= 2^31");
    ex.p[l] = operands[k];
    ex.ld[l] = static_cast<int>(lds[k]);
    code |= modes[k] << (2 * l);
  }
  ex.code = code;
  return aggregate_impl(indptr, indices, n_rows, nnz, GTA_IDX_EDGE, ex.p[0], F, F, GTA_F32, nullptr, 0, 0, nullptr,
                        y, ldy, 0, plan, plan_chunk, workspace, stream, nullptr, 0, nullptr, 0, &ex, XM_EX1 + shape - 1);
}

int gta_aggregate_self(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int x_mode,
                       const void* x, int64_t ldx, int64_t F, int x_dtype, const float* w, int64_t ldw, int64_t heads,
                       const float* row_scale, const void* x_self, int64_t ld_self, const float* self_scale, void* y,
                       int64_t ldy, int y_dtype, const void* plan, int64_t plan_chunk, void* workspace, void* stream) {
  if (!x_self) return fail(GTA_ERR_ARG, "aggregate_self: x_self is NULL");
  if (y_dtype != GTA_F32 && y_dtype != GTA_BF16) return fail(GTA_ERR_ARG, "aggregate_self: y_dtype must be F32 or BF16");
  return aggregate_impl(indptr, indices, n_rows, nnz, x_mode, x, ldx, F, x_dtype, w, ldw, heads, row_scale,
                        static_cast<float*>(y), ldy, 0, plan, plan_chunk, workspace, stream, x_self, ld_self, self_scale,
                        y_dtype == GTA_BF16 ? 1 : 0);
}

int64_t gta_aggregate_blocked_plan_bytes(int64_t n_rows, int64_t nnz, int64_t blocks, int64_t item_edges) {
  if (n_rows < 0 || nnz < 0 || blocks < 1 || blocks > 63 || item_edges < 1)
    return fail(GTA_ERR_ARG, "blocked_plan_bytes: need n_rows, nnz >= 0, 1 <= blocks <= 63, item_edges >= 1");
  const int B = static_cast<int>(blocks);
  return blocked_bytes(n_rows, B, blocked_max_items(n_rows, nnz, B, item_edges));
}

int gta_aggregate_blocked_plan_build(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                     int64_t nnz, int64_t blocks, int64_t item_edges, int64_t row_edges, void* plan,
                                     int64_t plan_bytes, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (!indptr || !plan || n_rows <= 0 || n_cols <= 0 || nnz < 0 || blocks < 1 || blocks > 63 || item_edges < 1 ||
      row_edges < 0)
    return fail(GTA_ERR_ARG, "blocked_plan_build: bad arguments");
  if (nnz > 0 && !indices) return fail(GTA_ERR_ARG, "blocked_plan_build: indices needed");
  if (n_rows > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "blocked_plan_build: > 2^31 rows");
  const int B = static_cast<int>(blocks);
  const int64_t mi = blocked_max_items(n_rows, nnz, B, item_edges);
  if (mi > INT32_MAX || n_rows * B > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "blocked_plan_build: > 2^31 items");
  if (plan_bytes < blocked_bytes(n_rows, B, mi)) return fail(GTA_ERR_ARG, "blocked_plan_build: plan buffer too small");
  BlockedView v = blocked_view(plan, n_rows, B, mi);
  hipStream_t s = S(stream);
  const int64_t bsize = (n_cols + B - 1) / B;
  const int class_major = tuning().seg_class_major ? 1 : 0;
  const int64_t hdr[16] = {B, bsize, n_rows, 0, 0, item_edges, mi,
                           reinterpret_cast<char*>(v.row_items) - static_cast<char*>(plan), row_edges, class_major};
  GTA_HIP(hipMemcpyAsync(v.hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
  GTA_HIP(hipMemsetAsync(v.bucket, 0, 2 * 256 * 4, s));
  k_blocked_seg<<<row_grid(n_rows), dim3(kBlock), 0, s>>>(
      indptr, indices, n_rows, B, bsize, item_edges, row_edges, class_major, v);
  GTA_LAUNCHED("k_blocked_seg");
  k_blocked_scan<<<1, 64, 0, s>>>(v, B, class_major);
  GTA_LAUNCHED("k_blocked_scan");
  k_blocked_perm<<<dim3(static_cast<unsigned>((n_rows + 255) / 256)), dim3(256), 0, s>>>(indptr, n_rows, B, row_edges,
                                                                                         class_major, v);
  GTA_LAUNCHED("k_blocked_perm");
  scan_excl<int64_t>(v.row_ptr, n_rows, 1, nullptr, v.scan, s);  // items per row -> row_ptr
  GTA_LAUNCHED("scan_excl");
  const dim3 gk(static_cast<unsigned>((n_rows * B + 255) / 256));
  k_blocked_cnt<<<gk, dim3(256), 0, s>>>(n_rows, B, item_edges, row_edges, v);
  GTA_LAUNCHED("k_blocked_cnt");
  scan_excl<int32_t>(v.cnt, n_rows * B, 0, &v.hdr[4], v.scan, s);  // -> first item id, n_items
  GTA_LAUNCHED("scan_excl");
  GTA_HIP(hipMemsetAsync(v.lhist, 0, kMaxGroups * kLenBins * 4, s));
  k_blocked_items<<<gk, dim3(256), 0, s>>>(indptr, n_rows, B, item_edges, row_edges, v);
  GTA_LAUNCHED("k_blocked_items");
  if (mi > 0) {  // each group's items longest first (matched half-wave pairs; only item ids move)
    k_items_len_scan<<<1, kMaxGroups, 0, s>>>(v);
    GTA_LAUNCHED("k_items_len_scan");
    k_items_permute<<<dim3(static_cast<unsigned>((mi + 255) / 256)), dim3(256), 0, s>>>(v);
    GTA_LAUNCHED("k_items_permute");
    GTA_HIP(hipMemcpyAsync(v.items, v.items_tmp, mi * sizeof(SegItem), hipMemcpyDeviceToDevice, s));
  }
  return GTA_OK;
}

// workspace of gta_aggregate_blocked: the slab rows, one [F] fp32 partial per plan item

int64_t gta_aggregate_blocked_workspace_bytes(int64_t n_rows, int64_t nnz, int64_t blocks, int64_t F,
                                              int64_t item_edges) {
  if (n_rows < 0 || nnz < 0 || blocks < 1 || blocks > 63 || F <= 0 || item_edges < 1)
    return fail(GTA_ERR_ARG, "blocked_workspace_bytes: bad sizes");
  return blocked_max_items(n_rows, nnz, static_cast<int>(blocks), item_edges) * F * static_cast<int64_t>(sizeof(float));
}

// gta_aggregate_blocked (who "aggregate_blocked", GTA_F32) and gta_aggregate_blocked_x: one argument
// check, one dispatch; the fp32 launches are the instantiations they always were.  bf16 rows
// (xv, ldx in bf16 elements) take the multi-item forms only -- the <..., BF = true> twins of the
// fp32 launches; the scalar-prefetch form (seg_pf) has no bf16 twin and is not selected for them.
static int aggregate_blocked_impl(const std::string& who, const int64_t* indptr, const int32_t* indices, int64_t n_rows,
                                  int64_t n_cols, int64_t nnz, const void* xv, int64_t ldx, int64_t F, int x_dtype,
                                  const float* w, int64_t ldw, int64_t heads, const float* row_scale, float* y,
                                  int64_t ldy, int accumulate, const void* plan, int64_t blocks, int64_t item_edges,
                                  void* workspace, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || nnz < 0 || F <= 0 || blocks < 1 || blocks > 63 || item_edges < 1)
    return fail(GTA_ERR_ARG, who + ": bad sizes");
  if (x_dtype != GTA_F32 && x_dtype != GTA_BF16) return fail(GTA_ERR_ARG, who + ": x_dtype must be F32 or BF16");
  if (n_rows == 0) return GTA_OK;
  if (!indptr || !xv || !y || !plan) return fail(GTA_ERR_ARG, who + ": bad arguments");
  const bool bf = x_dtype == GTA_BF16;
  const float* x = static_cast<const float*>(xv);  // bf: bf16 rows, read as such by the BF kernels only
  int gl = 0, vw = 0;
  for (int c : {4, 2, 1}) {
    if (F == static_cast<int64_t>(kWave) * c && (bf || (ldx % c == 0 && aligned(x, 4 * c))) && ldy % c == 0 &&
        aligned(y, 4 * c)) {
      vw = c;
      break;
    }
  }
  if (!vw) return fail(GTA_ERR_UNSUPPORTED, who + ": F must be 64, 128 or 256 (one edge per wave row)");
  bool gl_ok = true;  // head layout of the one-item-per-wave forms
  if (w) {
    if (heads <= 0 || F % heads) return fail(GTA_ERR_ARG, who + ": heads must divide F");
    gl = static_cast<int>(F / heads) / vw;
    gl_ok = (F / heads) % vw == 0 && (gl == 4 || gl == 8 || gl == 16);
  }
  const std::string gl_msg = who + ": (F/heads)/VW must be 4, 8 or 16 (or quarter-wave lanes per head 1..16)";
  const BlockedCall c(plan, n_rows, nnz, blocks, item_edges, workspace, stream);
  if (!workspace && nnz > 0) return fail(GTA_ERR_ARG, who + ": needs the slab workspace");
  // one launch over the plan's items into per-item slab rows, then the ordered reduce
  const int vq = static_cast<int>(F / 16);
  const int lph = w ? static_cast<int>((F / heads) / vq) : 0;
  // multi-item waves (F = 64 / 256: four 16-lane items; F = 128: two 32-lane items, one 512-B row per
  // half-wave instruction) when rows are 16-B aligned and the heads fit the lanes; else one item per wave
  const bool quarter = (vq == 4 || vq == 8 || vq == 16) && ldx % (bf ? 8 : 4) == 0 && aligned(x, 16) &&
                       (!w || ((F / heads) % vq == 0 && lph >= 1 && 16 % lph == 0));
  if (bf && !quarter)  // the one-item-per-wave fallback (k_agg_seg2d) has no bf16 twin
    return fail(GTA_ERR_UNSUPPORTED, who + ": bf16 rows need x 16-B aligned, ldx % 8 == 0 and heads that fit the "
                                           "multi-item forms (F/heads a multiple of F/16, lanes per head dividing 16)");
  const int phase = tuning().seg_phase;
  const unsigned xe = bf ? 2u : 4u;  // bytes per gathered element
  // the generic G-lane form <VW, U, WEIGHTED, NT, no ATT, G, BF>, fp32 and bf16, weighted or not
  auto seg4 = [&](auto VW, auto U, auto NT, auto G, dim3 grid, int lanes_per_head) {
    with_bools([&](auto W, auto BF) {
      k_agg_seg4<VW(), U(), W(), NT(), false, -1, G(), false, BF()><<<grid, c.blk, 0, c.s>>>(
          indices, c.nit, x, ldx, w, ldw, lanes_per_head, c.slabs, c.its);
    }, w != nullptr, bf);
  };
  if (c.items == 0 || phase == 2) {
    // no edges: no items; the reduce below writes the (empty) rows (phase 2: the reduce only)
  } else if (quarter && vq == 8) {  // F = 128: half-wave items, 32 lanes x float4 (bf16: x 8 B)
    const int lph32 = w ? static_cast<int>((F / heads) / 4) : 0;
    const bool lean = tuning().seg_lean && lean32_ok(n_cols, ldx, xe) &&
                      (!w || lph32 == 4 || (heads == 1 && tuning().seg_lean_w1 && ldw < (int64_t(1) << 24)));
    const uint32_t rb = static_cast<uint32_t>(ldx * xe);
    // NT template bits: 1 = non-temporal index loads, 2 = non-temporal slab stores (measured -0.5 % / -1 %;
    // non-temporal weight loads +3 %: profiles/r02_nt_bits_ab.json)
    if (lean) {
      const bool a1 = w && heads == 8 && ldw % 2 == 0 && aligned(w, 8) && tuning().seg_alpha1 &&
                      static_cast<uint64_t>(nnz) * static_cast<uint64_t>(ldw) * 4u < (1ull << 32);
      // the A1 walk on the edge grid: its aligned windows are whole 128-B lines of w and indices
      const bool grid = a1 && ldw == 8 && aligned(w, 128) && aligned(indices, 128) && tuning().seg_grid;
      const int pf = tuning().seg_pf;
      const uint32_t wbytes = static_cast<uint32_t>(nnz * ldw * 4), ibytes = static_cast<uint32_t>(nnz * 4);
      auto h32 = [&](auto W, auto NT, auto W1, auto A1) {  // k_agg_h32<WEIGHTED, NT, W1, A1, BF>
        with_bools([&](auto BF) {
          k_agg_h32<W(), NT(), W1(), A1(), BF()><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, w, ldw, c.slabs, c.its);
        }, bf);
      };
      constexpr BC<true> yes{};
      constexpr BC<false> no{};
      if (w && heads == 1) h32(yes, IC<2>{}, yes, no);
      else if (!bf && a1 && ldw == 8 && pf >= 1 && pf <= 5) {  // the scalar-prefetch form has no bf16 twin
#define GTA_PF(PFB_, PD_) \
  k_agg_h32pf<3, PFB_, PD_><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, w, ldw, c.slabs, c.its, wbytes, ibytes)
        if (pf == 1) GTA_PF(64, 0); else if (pf == 2) GTA_PF(128, 0); else if (pf == 3) GTA_PF(64, 1); else if (pf == 4) GTA_PF(128, 1);
        else k_agg_h32pf<3, 64, 0, 8><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, w, ldw, c.slabs, c.its, wbytes, ibytes);
#undef GTA_PF
      } else if (grid) {
        with_bools([&](auto BF) {
          k_agg_h32<true, 3, false, true, BF(), true><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, w, ldw, c.slabs,
                                                                                c.its, static_cast<uint32_t>(nnz));
        }, bf);
      } else if (a1) h32(yes, IC<3>{}, no, yes);
      else if (w) h32(yes, IC<3>{}, no, no);
      else h32(no, IC<2>{}, no, no);
      GTA_LAUNCHED("k_agg_h32");
    } else {
      seg4(IC<4>{}, IC<8>{}, IC<2>{}, IC<32>{}, c.g2h, lph32);
      GTA_LAUNCHED("k_agg_seg4<half>");
    }
  } else if (quarter) {  // F = 64 / 256: quarter-wave items
    if (vq == 4) seg4(IC<4>{}, IC<4>{}, IC<0>{}, IC<16>{}, c.g4, lph);
    else seg4(IC<16>{}, IC<2>{}, IC<0>{}, IC<16>{}, c.g4, lph);
    GTA_LAUNCHED("k_agg_seg4");
  } else {
    if (!gl_ok) return fail(GTA_ERR_UNSUPPORTED, gl_msg);
#define GTA_SEG2D(VW_, GL_) \
  k_agg_seg2d<VW_, GL_><<<c.g2, c.blk, 0, c.s>>>(indices, c.nit, x, ldx, w, ldw, c.slabs, c.its)
    if (vw == 2) {
      if (gl == 0) GTA_SEG2D(2, 0); else if (gl == 4) GTA_SEG2D(2, 4); else if (gl == 8) GTA_SEG2D(2, 8); else GTA_SEG2D(2, 16);
    } else if (vw == 4) {
      if (gl == 0) GTA_SEG2D(4, 0); else if (gl == 4) GTA_SEG2D(4, 4); else if (gl == 8) GTA_SEG2D(4, 8); else GTA_SEG2D(4, 16);
    } else {
      if (gl == 0) GTA_SEG2D(1, 0); else if (gl == 4) GTA_SEG2D(1, 4); else if (gl == 8) GTA_SEG2D(1, 8); else GTA_SEG2D(1, 16);
    }
#undef GTA_SEG2D
    GTA_LAUNCHED("k_agg_seg2d");
  }
  if (phase == 1) return GTA_OK;  // the item launch only; a later phase-2 call reduces
  dispatch_vw(vw, [&](auto V) {
    k_seg_reduce<V()><<<c.g3, c.blk, 0, c.s>>>(n_rows, c.slabs, row_scale, y, ldy, accumulate, c.ri);
  });
  GTA_LAUNCHED("k_seg_reduce");
  return GTA_OK;
}

int gta_aggregate_blocked(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, int64_t nnz,
                          const float* x, int64_t ldx, int64_t F, const float* w, int64_t ldw, int64_t heads,
                          const float* row_scale, float* y, int64_t ldy, int accumulate, const void* plan,
                          int64_t blocks, int64_t item_edges, void* workspace, void* stream) {
  return aggregate_blocked_impl("aggregate_blocked", indptr, indices, n_rows, n_cols, nnz, x, ldx, F, GTA_F32, w, ldw,
                                heads, row_scale, y, ldy, accumulate, plan, blocks, item_edges, workspace, stream);
}

int gta_aggregate_blocked_x(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, int64_t nnz,
                            const void* x, int64_t ldx, int64_t F, int x_dtype, const float* w, int64_t ldw,
                            int64_t heads, const float* row_scale, float* y, int64_t ldy, int accumulate,
                            const void* plan, int64_t blocks, int64_t item_edges, void* workspace, void* stream) {
  return aggregate_blocked_impl("aggregate_blocked_x", indptr, indices, n_rows, n_cols, nnz, x, ldx, F, x_dtype, w,
                                ldw, heads, row_scale, y, ldy, accumulate, plan, blocks, item_edges, workspace, stream);
}

// gta_reduce_blocked: one argument check, one dispatch.  MAX / MIN launch the k_red_* twins of the
// unweighted multi-item forms over the blocked plan's items, then k_seg_reduce_red; ADD is the
// blocked aggregate itself.
int gta_reduce_blocked(int red, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                       int64_t nnz, const void* xv, int64_t ldx, int64_t F, int x_dtype, float* y, int64_t ldy,
                       const void* plan, int64_t blocks, int64_t item_edges, void* workspace, void* stream) {
  const std::string who = "reduce_blocked";
  if (red != GTA_RED_ADD && red != GTA_RED_MAX && red != GTA_RED_MIN)
    return fail(GTA_ERR_ARG, who + ": red must be GTA_RED_ADD, GTA_RED_MAX or GTA_RED_MIN");
  if (x_dtype != GTA_F32 && x_dtype != GTA_BF16) return fail(GTA_ERR_ARG, who + ": x_dtype must be F32 or BF16");
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || F <= 0 || blocks < 1 || blocks > 63 || item_edges < 1)
    return fail(GTA_ERR_ARG, who + ": bad sizes (1 <= blocks <= 63, item_edges >= 1)");
  if (n_rows == 0) return GTA_OK;
  if (!indptr || !y || !plan || ldy < F) return fail(GTA_ERR_ARG, who + ": bad arguments");
  if (nnz > 0 && (!indices || !xv || !workspace || ldx < F))
    return fail(GTA_ERR_ARG, who + ": indices, x (ldx >= F) and the slab workspace are needed when nnz > 0");
  if (red == GTA_RED_ADD) {  // the sum is the blocked aggregate's: no weights, no row scale, no accumulate
    if (nnz == 0) { xv = y; ldx = ldy; x_dtype = GTA_F32; }  // any valid address: there is no item to read it
    const int rc = aggregate_blocked_impl(who + " (ADD)", indptr, indices, n_rows, n_cols, nnz, xv, ldx, F, x_dtype,
                                          nullptr, 0, 0, nullptr, y, ldy, 0, plan, blocks, item_edges, workspace, stream);
    return rc;
  }
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  const bool bf = x_dtype == GTA_BF16;
  int vw = 0;
  for (int c : {4, 2, 1})
    if (F == static_cast<int64_t>(kWave) * c && ldy % c == 0 && aligned(y, 4 * c)) { vw = c; break; }
  if (!vw) return fail(GTA_ERR_UNSUPPORTED, who + ": F must be 64, 128 or 256 with y rows aligned to F/64 floats");
  if (nnz > 0 && (ldx % (bf ? 8 : 4) != 0 || !aligned(xv, 16)))  // multi-item forms only: no one-item-per-wave twin
    return fail(GTA_ERR_UNSUPPORTED, who + ": x must be 16-B aligned with ldx % 4 == 0 (fp32) or ldx % 8 == 0 (bf16)");
  const BlockedCall c(plan, n_rows, nnz, blocks, item_edges, workspace, stream);
  const float* x = static_cast<const float*>(xv);  // bf: bf16 rows, read as such by the BF kernels only
  const uint32_t sbit = red == GTA_RED_MIN ? 0x80000000u : 0u;
  const unsigned xe = bf ? 2u : 4u;  // bytes per gathered element
  auto seg4 = [&](auto VW, auto U, auto G, dim3 grid) {  // k_red_seg4<VW, U, G, BF>
    with_bools([&](auto BF) {
      k_red_seg4<VW(), U(), G(), BF()><<<grid, c.blk, 0, c.s>>>(indices, c.nit, x, ldx, sbit, c.slabs, c.its);
    }, bf);
  };
  if (c.items == 0) {
    // no edges: no items; the reduce below writes the (empty) rows
  } else if (F == 128) {  // half-wave items
    if (tuning().seg_lean && lean32_ok(n_cols, ldx, xe)) {
      const uint32_t rb = static_cast<uint32_t>(ldx * xe);
      with_bools([&](auto BF) {
        k_red_h32<2, BF()><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, sbit, c.slabs, c.its);
      }, bf);
      GTA_LAUNCHED("k_red_h32");
    } else {
      seg4(IC<4>{}, IC<8>{}, IC<32>{}, c.g2h);
      GTA_LAUNCHED("k_red_seg4<half>");
    }
  } else {  // F = 64 / 256: quarter-wave items
    if (F == 64) seg4(IC<4>{}, IC<4>{}, IC<16>{}, c.g4);
    else seg4(IC<16>{}, IC<2>{}, IC<16>{}, c.g4);
    GTA_LAUNCHED("k_red_seg4");
  }
  dispatch_vw(vw, [&](auto V) {
    k_seg_reduce_red<V()><<<c.g3, c.blk, 0, c.s>>>(n_rows, c.slabs, sbit, y, ldy, c.ri);
  });
  GTA_LAUNCHED("k_seg_reduce_red");
  return GTA_OK;
}

int64_t gta_gat_aggregate_blocked_workspace_bytes(int64_t n_rows, int64_t nnz, int64_t blocks, int64_t F,
                                                  int64_t heads, int64_t item_edges) {
  if (n_rows < 0 || nnz < 0 || blocks < 1 || blocks > 63 || F <= 0 || heads <= 0 || item_edges < 1)
    return fail(GTA_ERR_ARG, "gat_workspace_bytes: bad sizes");
  return blocked_max_items(n_rows, nnz, static_cast<int>(blocks), item_edges) * (F + ((heads + 3) & ~3)) *
         static_cast<int64_t>(sizeof(float));
}

// gta_gat_aggregate_blocked (shifted false), gta_gat_aggregate_blocked_shifted and
// gta_gat_aggregate_blocked_x: one argument check, one dispatch; the fp32 launches are the
// instantiations they always were, bf16 rows (xv, ldx in bf16 elements) launch their <..., BF = true> twins.
static int gat_aggregate_blocked_impl(const char* who, bool shifted, const int64_t* indptr, const int32_t* indices,
                                      int64_t n_rows, int64_t n_cols, int64_t nnz, const void* xv, int64_t ldx,
                                      int64_t F, int x_dtype, const float* a_dst, int64_t lda, const float* b_src, int64_t ldb,
                                      int64_t heads, int sf, int normalize, int sf_out, float* y, int64_t ldy,
                                      float* sums, const void* plan, int64_t blocks, int64_t item_edges,
                                      void* workspace, const float* shift, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || nnz < 0 || blocks < 1 || blocks > 63 || heads <= 0 || lda < heads || ldb < heads ||
      item_edges < 1 || sf_out < GTA_SF_NONE || sf_out > GTA_SF_RECIP)
    return fail(GTA_ERR_ARG, std::string(who) + ": bad sizes");
  if (x_dtype != GTA_F32 && x_dtype != GTA_BF16)
    return fail(GTA_ERR_ARG, std::string(who) + ": x_dtype must be F32 or BF16");
  const bool bf = x_dtype == GTA_BF16;
  const float* x = static_cast<const float*>(xv);  // bf: bf16 rows, read as such by the BF kernels only
  if (shifted && !shift) return fail(GTA_ERR_ARG, std::string(who) + ": shift is required");
  if (shifted && !sf_is_exp_form(sf))
    return fail(GTA_ERR_UNSUPPORTED, std::string(who) + ": sf must be EXP_LEAKY_RELU or EXP");
  if (n_rows == 0) return GTA_OK;
  if (!indptr || !x || !a_dst || !b_src || !y || !plan || (!workspace && nnz > 0))
    return fail(GTA_ERR_ARG, std::string(who) + ": bad arguments");
  const int vq = static_cast<int>(F / 16);
  if ((F != 64 && F != 128 && F != 256) || F % heads || (F / heads) % vq || ldx % (bf ? 8 : 4) || !aligned(x, 16) ||
      ldy % (F / 64) || !aligned(y, 4 * (F / 64)))
    return fail(GTA_ERR_UNSUPPORTED, std::string(who) + ": F in {64,128,256}, 16-B rows (bf16: ldx % 8 == 0), F/heads "
                                                          "a multiple of F/16");
  const int lph = static_cast<int>((F / heads) / vq);
  if (lph < 1 || 16 % lph) return fail(GTA_ERR_UNSUPPORTED, std::string(who) + ": lanes per head must divide 16");
  const BlockedCall c(plan, n_rows, nnz, blocks, item_edges, workspace, stream);
  AttArgs att{a_dst, lda, b_src, ldb, sf, static_cast<int>(heads), shift};
  int skip_single = 0;  // rows whose only item wrote y directly (k_att_h32)
  if (c.items > 0) {  // no edges: no items, the reduce alone writes the empty rows
    const bool elr = sf == GTA_SF_EXP_LEAKY_RELU;  // GAT's score function, specialised
    const unsigned xe = bf ? 2u : 4u;              // bytes per gathered element
    // the generic G-lane attention form <VW, U, ATT, SFC (elr fixed at compile time), G, SH, BF>
    auto seg4 = [&](auto VW, auto U, auto G, dim3 grid, int lanes_per_head) {
      with_bools([&](auto ELR, auto SH, auto BF) {
        k_agg_seg4<VW(), U(), false, 0, true, (ELR() ? GTA_SF_EXP_LEAKY_RELU : -1), G(), SH(), BF()>
            <<<grid, c.blk, 0, c.s>>>(indices, c.nit, x, ldx, nullptr, 0, lanes_per_head, c.slabs, c.its, att);
      }, elr, shifted, bf);
    };
    const int lph32 = static_cast<int>((F / heads) / 4);
    const bool lean = tuning().att_lean && elr && F == 128 && heads == 8 && lean32_ok(n_cols, ldx, xe) &&
                      lean32_ok(n_cols, ldb, 4u);
    if (lean) {
      const uint32_t rb = static_cast<uint32_t>(ldx * xe), bbytes = static_cast<uint32_t>(ldb * 4);
      // single-item rows are common only when few blocks cut the rows (low degree, B <= 2); above
      // that the row_ptr reads at every item's end cost more than the rare direct writes save
      const bool direct = (tuning().att_direct == 2 || (tuning().att_direct == 1 && blocks <= 2)) && ldy % 4 == 0 &&
                          aligned(y, 16);
      skip_single = direct;
      const int64_t* rp = direct ? c.v.row_ptr : nullptr;
      with_bools([&](auto SH, auto BF) {  // NT bit 2: non-temporal slab stores; shift is NULL unless shifted
        k_att_h32<2, SH(), BF()><<<c.g2h, c.blk, 0, c.s>>>(indices, c.nit, x, rb, a_dst, lda, b_src, bbytes, c.slabs,
                                                           c.its, rp, normalize, y, ldy, sums, sf_out, shift);
      }, shifted, bf);
    } else if (F == 128 && (F / heads) % 4 == 0 && lph32 >= 1 && 32 % lph32 == 0) {
      seg4(IC<4>{}, IC<8>{}, IC<32>{}, c.g2h, lph32);
    } else if (vq == 4) {
      seg4(IC<4>{}, IC<4>{}, IC<16>{}, c.g4, lph);
    } else {
      seg4(IC<16>{}, IC<2>{}, IC<16>{}, c.g4, lph);
    }
    GTA_LAUNCHED("k_agg_seg4<att>");
  }
  const int H = static_cast<int>(heads);
  dispatch_vw(static_cast<int>(F / 64), [&](auto V) {  // skip_single is set at F = 128 only
    k_seg_reduce_att<V()><<<c.g3, c.blk, 0, c.s>>>(n_rows, c.slabs, H, normalize, y, ldy, sums, c.ri, skip_single, sf_out);
  });
  GTA_LAUNCHED("k_seg_reduce_att");
  return GTA_OK;
}

int gta_gat_aggregate_blocked(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                              int64_t nnz, const float* x, int64_t ldx, int64_t F, const float* a_dst, int64_t lda,
                              const float* b_src, int64_t ldb, int64_t heads, int sf, int normalize, int sf_out,
                              float* y, int64_t ldy, float* sums, const void* plan, int64_t blocks, int64_t item_edges,
                              void* workspace, void* stream) {
  return gat_aggregate_blocked_impl("gat_aggregate_blocked", false, indptr, indices, n_rows, n_cols, nnz, x, ldx, F,
                                    GTA_F32, a_dst, lda, b_src, ldb, heads, sf, normalize, sf_out, y, ldy, sums, plan, blocks,
                                    item_edges, workspace, nullptr, stream);
}

int gta_gat_aggregate_blocked_shifted(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                      int64_t nnz, const float* x, int64_t ldx, int64_t F, const float* a_dst,
                                      int64_t lda, const float* b_src, int64_t ldb, int64_t heads, int sf,
                                      int normalize, int sf_out, float* y, int64_t ldy, float* sums, const void* plan,
                                      int64_t blocks, int64_t item_edges, void* workspace, const float* shift,
                                      void* stream) {
  return gat_aggregate_blocked_impl("gat_aggregate_blocked_shifted", true, indptr, indices, n_rows, n_cols, nnz, x,
                                    ldx, F, GTA_F32, a_dst, lda, b_src, ldb, heads, sf, normalize, sf_out, y, ldy, sums,
                                    plan, blocks, item_edges, workspace, shift, stream);
}

int gta_gat_aggregate_blocked_x(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols,
                                int64_t nnz, const void* x, int64_t ldx, int64_t F, int x_dtype, const float* a_dst,
                                int64_t lda, const float* b_src, int64_t ldb, int64_t heads, int sf, int normalize,
                                int sf_out, float* y, int64_t ldy, float* sums, const void* plan, int64_t blocks,
                                int64_t item_edges, void* workspace, const float* shift, void* stream) {
  return gat_aggregate_blocked_impl("gat_aggregate_blocked_x", shift != nullptr, indptr, indices, n_rows, n_cols, nnz,
                                    x, ldx, F, x_dtype, a_dst, lda, b_src, ldb, heads, sf, normalize, sf_out, y, ldy,
                                    sums, plan, blocks, item_edges, workspace, shift, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// CSC view of the CSR (ABI 11): the edge permutation that orders edges by SOURCE column, for the
// ISA gather with DIRECTION src (template/ISA_defination.yaml:46-48, "from edges to src
// (column-wise)"; lowered with ORDER C, code/interpreter.py:108-121).  A stable LSD radix sort of
// (source column, edge id) with 8-bit digits: per pass a per-tile digit histogram, one exclusive
// scan over [digit][tile], and a stable scatter in which every element's place is fixed by its
// position in the CSR (ranks inside a wave from 8 ballots, across waves and rounds from LDS
// counters) -- no atomics decide an order, so perm is a pure function of the graph: within a
// column, edges keep CSR order (increasing destination row, then CSR position).
// ---------------------------------------------------------------------------
namespace {
constexpr int kRadixItems = 16;                    // elements per thread per tile
constexpr int64_t kRadixTile = int64_t{kBlock} * kRadixItems;

__global__ void __launch_bounds__(kBlock) k_radix_hist(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                       int32_t* __restrict__ hist, int64_t nb) {
  __shared__ uint32_t cnt[256];
  const int t = threadIdx.x;
  cnt[t] = 0;
  __syncthreads();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kRadixTile;
#pragma unroll 4
  for (int r = 0; r < kRadixItems; ++r) {
    const int64_t i = base + r * kBlock + t;
    if (i < n) atomicAdd(&cnt[(keys[i] >> shift) & 255u], 1u);  // a count: order-independent
  }
  __syncthreads();
  hist[static_cast<int64_t>(t) * nb + blockIdx.x] = static_cast<int32_t>(cnt[t]);
}

// vals_in == nullptr: the value of element i is i (the edge id, first pass)
__global__ void __launch_bounds__(kBlock) k_radix_scatter(const uint32_t* __restrict__ keys_in,
                                                          const uint32_t* __restrict__ vals_in, int64_t n, int shift,
                                                          const int32_t* __restrict__ offs, int64_t nb,
                                                          uint32_t* __restrict__ keys_out,
                                                          uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t run[256];
  __shared__ uint32_t wcnt[kWavesPerBlock][256];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  run[t] = static_cast<uint32_t>(offs[static_cast<int64_t>(t) * nb + blockIdx.x]);
#pragma unroll
  for (int q = 0; q < kWavesPerBlock; ++q) wcnt[q][t] = 0;
  __syncthreads();
  const uint64_t below = lane ? (~0ull >> (kWave - lane)) : 0ull;
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kRadixTile;
  for (int r = 0; r < kRadixItems; ++r) {  // round r: elements base + r*256 + t, in thread order
    const int64_t i = base + r * kBlock + t;
    const bool valid = i < n;
    const uint32_t k = valid ? keys_in[i] : 0u;
    const uint32_t v = valid ? (vals_in ? vals_in[i] : static_cast<uint32_t>(i)) : 0u;
    const uint32_t d = (k >> shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t rank = static_cast<uint32_t>(__popcll(peers & below));
    const uint32_t cnt = static_cast<uint32_t>(__popcll(peers));
    if (valid && rank + 1 == cnt) wcnt[w][d] = cnt;  // the wave's last lane of this digit
    __syncthreads();
    if (valid) {
      uint32_t pos = run[d] + rank;
      for (int q = 0; q < w; ++q) pos += wcnt[q][d];
      if (keys_out) keys_out[pos] = k;
      vals_out[pos] = v;
    }
    __syncthreads();
    uint32_t add = 0;
#pragma unroll
    for (int q = 0; q < kWavesPerBlock; ++q) {
      add += wcnt[q][t];
      wcnt[q][t] = 0;
    }
    run[t] += add;
    __syncthreads();
  }
}

// colptr[j] = first position of column j in the sorted keys (lower bound), j in [0, n_cols]
__global__ void __launch_bounds__(kBlock) k_csc_colptr(const uint32_t* __restrict__ sorted, int64_t n, int64_t n_cols,
                                                       int64_t* __restrict__ colptr) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j > n_cols) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(sorted[mid]) < j) lo = mid + 1; else hi = mid;
  }
  colptr[j] = lo;
}

// rows[k] = destination row of edge perm[k] (the last row whose indptr start is <= perm[k])
__global__ void __launch_bounds__(kBlock) k_csc_rows(const int64_t* __restrict__ indptr, int64_t n_rows,
                                                     const int32_t* __restrict__ perm, int64_t n,
                                                     int32_t* __restrict__ rows) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= n) return;
  const int64_t e = perm[k];
  int64_t lo = 0, hi = n_rows;  // invariant: indptr[lo] <= e < indptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (indptr[mid] <= e) lo = mid; else hi = mid;
  }
  rows[k] = static_cast<int32_t>(lo);
}

struct CscWork {
  uint32_t* keys[2];
  uint32_t* vals;
  int32_t* hist;
  int64_t* scan;
  int64_t nb;
};

inline int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

int64_t csc_layout(int64_t nnz, char* p, CscWork* w) {
  const int64_t nb = (nnz + kRadixTile - 1) / kRadixTile;
  const int64_t kb = round256(nnz * 4), hb = round256((256 * nb + 1) * 4), sb = round256((kScanMaxTiles + 1) * 8);
  if (w) {
    w->keys[0] = reinterpret_cast<uint32_t*>(p);
    w->keys[1] = reinterpret_cast<uint32_t*>(p + kb);
    w->vals = reinterpret_cast<uint32_t*>(p + 2 * kb);
    w->hist = reinterpret_cast<int32_t*>(p + 3 * kb);
    w->scan = reinterpret_cast<int64_t*>(p + 3 * kb + hb);
    w->nb = nb;
  }
  return 3 * kb + hb + sb;
}
}  // namespace

extern "C" {

int64_t gta_csc_workspace_bytes(int64_t n_cols, int64_t nnz) {
  if (n_cols < 0 || nnz < 0) return -1;
  return csc_layout(nnz, nullptr, nullptr);
}

int gta_csc_build(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, int64_t nnz,
                  int64_t* colptr, int32_t* perm, int32_t* rows, void* workspace, int64_t workspace_bytes,
                  void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || !colptr) return fail(GTA_ERR_ARG, "csc_build: bad arguments");
  if (nnz > INT32_MAX) return fail(GTA_ERR_UNSUPPORTED, "csc_build: more than 2^31 - 1 edges");
  if (n_cols > (int64_t{1} << 32)) return fail(GTA_ERR_UNSUPPORTED, "csc_build: more than 2^32 columns");
  hipStream_t s = S(stream);
  if (nnz == 0) {
    GTA_HIP(hipMemsetAsync(colptr, 0, (n_cols + 1) * sizeof(int64_t), s));
    return GTA_OK;
  }
  if (!indptr || !indices || !perm || n_rows == 0 || n_cols == 0) return fail(GTA_ERR_ARG, "csc_build: bad arguments");
  if (!workspace || workspace_bytes < csc_layout(nnz, nullptr, nullptr))
    return fail(GTA_ERR_ARG, "csc_build: workspace smaller than gta_csc_workspace_bytes");
  CscWork w;
  csc_layout(nnz, static_cast<char*>(workspace), &w);
  int bits = 0;
  for (uint64_t m = static_cast<uint64_t>(n_cols - 1); m; m >>= 1) ++bits;
  const int passes = bits > 8 ? (bits + 7) / 8 : 1;
  const dim3 grid(static_cast<unsigned>(w.nb)), blk(kBlock);
  const uint32_t* kin = reinterpret_cast<const uint32_t*>(indices);
  const uint32_t* vin = nullptr;
  for (int p = 0; p < passes; ++p) {
    uint32_t* kout = w.keys[p & 1];
    uint32_t* vout = ((passes - 1 - p) % 2 == 0) ? reinterpret_cast<uint32_t*>(perm) : w.vals;  // last pass -> perm
    k_radix_hist<<<grid, blk, 0, s>>>(kin, nnz, 8 * p, w.hist, w.nb);
    GTA_LAUNCHED("k_radix_hist");
    scan_excl<int32_t>(w.hist, 256 * w.nb, 0, nullptr, w.scan, s);
    GTA_LAUNCHED("scan_excl");
    k_radix_scatter<<<grid, blk, 0, s>>>(kin, vin, nnz, 8 * p, w.hist, w.nb, kout, vout);
    GTA_LAUNCHED("k_radix_scatter");
    kin = kout;
    vin = vout;
  }
  k_csc_colptr<<<dim3(static_cast<unsigned>((n_cols + 1 + kBlock - 1) / kBlock)), blk, 0, s>>>(kin, nnz, n_cols, colptr);
  GTA_LAUNCHED("k_csc_colptr");
  if (rows) {
    k_csc_rows<<<dim3(static_cast<unsigned>((nnz + kBlock - 1) / kBlock)), blk, 0, s>>>(indptr, n_rows, perm, nnz, rows);
    GTA_LAUNCHED("k_csc_rows");
  }
  return GTA_OK;
}

int gta_gather_add(int dir, const int64_t* indptr, int64_t n_rows, int64_t nnz, const int64_t* colptr,
                   const int32_t* perm, int64_t n_cols, const float* xe, int64_t ldxe, int64_t F, float* y,
                   int64_t ldy, int accumulate, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (dir == GTA_DIR_R)
    return gta_aggregate(indptr, nullptr, n_rows, nnz, GTA_IDX_EDGE, xe, ldxe, F, GTA_F32, nullptr, 0, 0, nullptr, y,
                         ldy, accumulate, nullptr, 0, nullptr, stream);
  if (dir != GTA_DIR_C) return fail(GTA_ERR_ARG, "gather_add: bad dir");
  if (n_cols < 0) return fail(GTA_ERR_ARG, "gather_add: bad n_cols");
  if (nnz > 0 && (!colptr || !perm)) return fail(GTA_ERR_ARG, "gather_add C needs the CSC view (gta_csc_build)");
  if (nnz == 0 && n_cols > 0 && !colptr) return fail(GTA_ERR_ARG, "gather_add C needs colptr");
  // y[j] = sum over column j's edges, in CSC order, of xe[perm[k]]: the edge tensor read as a table
  // of nnz rows gathered by index -- the same ordered row kernel as direction R, no atomics
  return gta_aggregate(colptr, perm, n_cols, nnz, GTA_IDX_SRC, xe, ldxe, F, GTA_F32, nullptr, 0, 0, nullptr, y, ldy,
                       accumulate, nullptr, 0, nullptr, stream);
}

int gta_scatter(int dir, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const void* x,
                int64_t ldx, int64_t F, int dtype, void* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || nnz < 0 || F <= 0) return fail(GTA_ERR_ARG, "scatter: bad sizes");
  if (dir != GTA_DIR_R && dir != GTA_DIR_C) return fail(GTA_ERR_ARG, "scatter: bad dir");
  const int esz = (dtype == GTA_BF16) ? 2 : (dtype == GTA_F32 ? 4 : 0);
  if (!esz) return fail(GTA_ERR_ARG, "scatter: bad dtype");
  if (n_rows == 0 || nnz == 0) return GTA_OK;
  if (!indptr || !x || !out) return fail(GTA_ERR_ARG, "scatter: bad arguments");
  if (dir == GTA_DIR_C && !indices) return fail(GTA_ERR_ARG, "scatter C needs indices");
  const int64_t rowb = F * esz, ldxb = ldx * esz, ldob = ldo * esz;
  int unit = 16;
  while (unit > 2 && (rowb % unit || ldxb % unit || ldob % unit || !aligned(x, unit) || !aligned(out, unit))) unit >>= 1;
  const auto launch = [&](auto u) {  // u: a value of the copy unit's type
    using UNIT = decltype(u);
    constexpr int64_t ub = sizeof(UNIT);
    k_scatter<UNIT><<<row_grid(n_rows), dim3(kBlock), 0, S(stream)>>>(dir, indptr, indices, n_rows,
                                                                      static_cast<const UNIT*>(x), ldxb / ub, rowb / ub,
                                                                      static_cast<UNIT*>(out), ldob / ub);
  };
  if (unit == 16) launch(uint4{});
  else if (unit == 8) launch(uint2{});
  else if (unit == 4) launch(uint32_t{});
  else launch(uint16_t{});
  GTA_LAUNCHED("k_scatter");
  return GTA_OK;
}

static int check_bcast(int64_t Fa, int64_t Fb, bool has_b, int64_t* Fo) {
  *Fo = Fa;
  if (!has_b) return 0;
  *Fo = Fa > Fb ? Fa : Fb;
  if (Fa <= 0 || Fb <= 0 || (*Fo % Fa) || (*Fo % Fb)) return -1;
  return 0;
}

int gta_apply_edge(int bin, int sf, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                   const float* a, int a_mode, int64_t lda, int64_t Fa, const float* b, int b_mode, int64_t ldb,
                   int64_t Fb, float* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n_rows < 0 || nnz < 0 || Fa <= 0) return fail(GTA_ERR_ARG, "apply_edge: bad sizes");
  if (n_rows == 0 || nnz == 0) return GTA_OK;  // no edge: nothing to write (operands may be NULL)
  if (!indptr || !a || !out) return fail(GTA_ERR_ARG, "apply_edge: bad arguments");
  if ((a_mode == GTA_IDX_SRC || (b && b_mode == GTA_IDX_SRC)) && !indices)
    return fail(GTA_ERR_ARG, "apply_edge: SRC operand needs indices");
  int64_t Fo;
  if (check_bcast(Fa, Fb, b != nullptr, &Fo)) return fail(GTA_ERR_ARG, "apply_edge: widths must divide");
  const dim3 grid = row_grid(n_rows);
  const int fo = static_cast<int>(Fo), ga = static_cast<int>(Fo / Fa), gb = b ? static_cast<int>(Fo / Fb) : 1;
  if (tuning().apply_edge_form == 0) {
    k_apply_edge<<<grid, dim3(kBlock), 0, S(stream)>>>(bin, sf, indptr, indices, n_rows, a, a_mode, lda,
                                                       static_cast<int>(Fa), b, b_mode, ldb, static_cast<int>(Fb),
                                                       out, ldo, fo);
  } else if (fo <= 32 && (fo & (fo - 1)) == 0) {
    k_apply_edge_pack<<<grid, dim3(kBlock), 0, S(stream)>>>(bin, sf, indptr, indices, n_rows, a, a_mode, lda, ga,
                                                            b, b_mode, ldb, gb, out, ldo, fo);
  } else {
    int vw = 1;  // the widest of 4, 2 that divides fo, fills a wave and is aligned
    for (int c : {2, 4})
      if (fo % c == 0 && fo >= c * kWave && vec_ok(c, a, lda, ga, b, ldb, gb, out, ldo)) vw = c;
    dispatch_vw(vw, [&](auto V) {
      k_apply_edge_cols<V.value><<<grid, dim3(kBlock), 0, S(stream)>>>(bin, sf, indptr, indices, n_rows, a, a_mode, lda,
                                                                       ga, b, b_mode, ldb, gb, out, ldo, fo);
    });
  }
  GTA_LAUNCHED("k_apply_edge");
  return GTA_OK;
}

int gta_apply_edge_flat(int bin, int sf, const int32_t* edge_rows, const int32_t* indices, int64_t nnz, const float* a,
                        int a_mode, int64_t lda, int64_t Fa, const float* b, int b_mode, int64_t ldb, int64_t Fb,
                        float* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (nnz < 0 || Fa <= 0) return fail(GTA_ERR_ARG, "apply_edge_flat: bad sizes");
  if (nnz == 0) return GTA_OK;
  if (!a || !out) return fail(GTA_ERR_ARG, "apply_edge_flat: bad arguments");
  const bool b_rows = b && ldb != 0;
  if ((a_mode == GTA_IDX_SRC || (b_rows && b_mode == GTA_IDX_SRC)) && !indices)
    return fail(GTA_ERR_ARG, "apply_edge_flat: SRC operand needs indices");
  if ((a_mode == GTA_IDX_DST || (b_rows && b_mode == GTA_IDX_DST)) && !edge_rows)
    return fail(GTA_ERR_ARG, "apply_edge_flat: DST operand needs edge_rows");
  int64_t Fo;
  if (check_bcast(Fa, Fb, b != nullptr, &Fo)) return fail(GTA_ERR_ARG, "apply_edge_flat: widths must divide");
  const int ga = static_cast<int>(Fo / Fa), gb = b ? static_cast<int>(Fo / Fb) : 1;
  int vw = 0;
  for (int c : {4, 2, 1})
    if (Fo == static_cast<int64_t>(kWave) * c) vw = c;
  if (!vw || !vec_ok(vw, a, lda, ga, b, ldb, gb, out, ldo))
    return fail(GTA_ERR_UNSUPPORTED, "apply_edge_flat: the output must be 64, 128 or 256 columns, rows aligned to them");
  const dim3 grid(static_cast<unsigned>((nnz + 32 * kWavesPerBlock - 1) / (32 * kWavesPerBlock)));
  dispatch_vw(vw, [&](auto V) {
    k_apply_edge_flat<V.value><<<grid, dim3(kBlock), 0, S(stream)>>>(bin, sf, edge_rows, indices, nnz, a, a_mode, lda,
                                                                     ga, b, b_mode, ldb, gb, out, ldo);
  });
  GTA_LAUNCHED("k_apply_edge_flat");
  return GTA_OK;
}

int gta_apply_node(int bin, int sf, int64_t n, const void* a, int64_t lda, int64_t Fa, int a_dtype, const float* b,
                   int64_t ldb, int64_t Fb, float* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (n < 0 || Fa <= 0) return fail(GTA_ERR_ARG, "apply_node: bad sizes");
  if (a_dtype != GTA_F32 && a_dtype != GTA_BF16) return fail(GTA_ERR_ARG, "apply_node: a_dtype must be F32 or BF16");
  if (n == 0) return GTA_OK;
  if (!a || !out) return fail(GTA_ERR_ARG, "apply_node: bad arguments");
  const bool bf = a_dtype == GTA_BF16;
  const float* af = static_cast<const float*>(a);
  const uint16_t* ah = static_cast<const uint16_t*>(a);
  int64_t Fo;
  if (check_bcast(Fa, Fb, b != nullptr, &Fo)) return fail(GTA_ERR_ARG, "apply_node: widths must divide");
  const int64_t total = n * Fo;
  const int bm = !b ? 0 : (Fb == Fo ? 1 : (Fb == 1 ? 2 : -1));
  if (tuning().apply_node_vec && bm >= 0 && Fa == Fo && Fo % 4 == 0 && total / 4 < (int64_t(1) << 32) && lda % 4 == 0 &&
      ldo % 4 == 0 && aligned(a, bf ? 8 : 16) && aligned(out, 16) && (bm != 1 || (ldb % 4 == 0 && aligned(b, 16)))) {
    const uint32_t n4 = static_cast<uint32_t>(total / 4), F4 = static_cast<uint32_t>(Fo / 4);
    const dim3 g(static_cast<unsigned>(std::min<int64_t>((n4 + kBlock - 1) / kBlock, 256 * 16))), blk(kBlock);
    const auto launch = [&](auto BM) {
      if (bf) k_apply_node4<BM.value, uint16_t><<<g, blk, 0, S(stream)>>>(bin, sf, n4, F4, ah, lda, b, ldb, out, ldo);
      else k_apply_node4<BM.value><<<g, blk, 0, S(stream)>>>(bin, sf, n4, F4, af, lda, b, ldb, out, ldo);
    };
    if (bm == 0) launch(IC<0>{});
    else if (bm == 1) launch(IC<1>{});
    else launch(IC<2>{});
    GTA_LAUNCHED("k_apply_node4");
    return GTA_OK;
  }
  const int64_t blocks = std::min<int64_t>((total + kBlock - 1) / kBlock, 256 * 16);
  const dim3 g(static_cast<unsigned>(blocks));
  if (bf)
    k_apply_node<uint16_t><<<g, dim3(kBlock), 0, S(stream)>>>(bin, sf, n, ah, lda, static_cast<int>(Fa), b, ldb,
                                                              static_cast<int>(Fb), out, ldo, static_cast<int>(Fo));
  else
    k_apply_node<float><<<g, dim3(kBlock), 0, S(stream)>>>(bin, sf, n, af, lda, static_cast<int>(Fa), b, ldb,
                                                           static_cast<int>(Fb), out, ldo, static_cast<int>(Fo));
  GTA_LAUNCHED("k_apply_node");
  return GTA_OK;
}

// gta_edge_softmax (shift NULL, shifted false) and gta_edge_softmax_shifted: one argument check, one
// dispatch; the unshifted launches are the instantiations they always were.
static int edge_softmax_impl(const char* who, bool shifted, const int64_t* indptr, const int32_t* indices,
                             int64_t n_rows, int64_t nnz, const float* a_dst, int64_t lda, const float* b_src,
                             int64_t ldb, int64_t heads, int sf, int normalize, float* out, float* sums,
                             const float* shift, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (!indptr || !a_dst || !b_src || n_rows < 0 || nnz < 0 || (nnz > 0 && (!indices || !out)) || (shifted && !shift))
    return fail(GTA_ERR_ARG, std::string(who) + ": bad arguments");
  if (const int rc = check_heads(who, heads, sf, shifted, lda, ldb)) return rc;
  if (n_rows == 0) return GTA_OK;
  const dim3 grid = row_grid(n_rows);
  const bool vec = tuning().esm_lane && (heads == 4 || heads == 8 || heads == 16) && ldb % 4 == 0 && aligned(b_src, 16) &&
                   (nnz == 0 || aligned(out, 16));
  if (vec) {
    // chunks of 64 edges held in VGPRs: 4 for H <= 8, 2 at H = 16 (register budget)
    const auto launch = [&](auto H, auto K) {
      with_bools([&](auto SH) {
        k_edge_softmax_v<H.value, K.value, SH.value><<<grid, dim3(kBlock), 0, S(stream)>>>(
            indptr, indices, n_rows, a_dst, lda, b_src, ldb, sf, normalize, out, sums, shift);
      }, shifted);
    };
    if (heads == 4) launch(IC<4>{}, IC<4>{});
    else if (heads == 8) launch(IC<8>{}, IC<4>{});
    else launch(IC<16>{}, IC<2>{});
    GTA_LAUNCHED("k_edge_softmax_v");
    return GTA_OK;
  }
  dispatch_heads(heads, [&](auto H) {
    with_bools([&](auto SH) {
      k_edge_softmax<H.value, SH.value><<<grid, dim3(kBlock), 0, S(stream)>>>(indptr, indices, n_rows, a_dst, lda, b_src,
                                                                              ldb, sf, normalize, out, sums, shift);
    }, shifted);
  });
  GTA_LAUNCHED("k_edge_softmax");
  return GTA_OK;
}

int gta_edge_softmax(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                     const float* a_dst, int64_t lda, const float* b_src, int64_t ldb, int64_t heads, int sf,
                     int normalize, float* out, float* sums, void* stream) {
  return edge_softmax_impl("edge_softmax", false, indptr, indices, n_rows, nnz, a_dst, lda, b_src, ldb, heads, sf,
                           normalize, out, sums, nullptr, stream);
}

int gta_edge_softmax_shifted(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz,
                             const float* a_dst, int64_t lda, const float* b_src, int64_t ldb, int64_t heads, int sf,
                             int normalize, float* out, float* sums, const float* shift, void* stream) {
  return edge_softmax_impl("edge_softmax_shifted", true, indptr, indices, n_rows, nnz, a_dst, lda, b_src, ldb, heads,
                           sf, normalize, out, sums, shift, stream);
}

int gta_softmax_shift(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const float* a_dst,
                      int64_t lda, const float* b_src, int64_t ldb, int64_t heads, int sf, float* shift,
                      void* stream) {
  if (!indptr || !a_dst || !shift || n_rows < 0 || nnz < 0 || (nnz > 0 && (!indices || !b_src)))
    return fail(GTA_ERR_ARG, "softmax_shift: bad arguments");
  if (const int rc = check_heads("softmax_shift", heads, sf, true, lda, ldb)) return rc;
  if (n_rows == 0) return GTA_OK;
  // nnz == 0: every degree is 0, the kernel writes zeros and reads neither indices nor b_src
  dispatch_heads(heads, [&](auto H) {
    k_softmax_shift<H.value><<<row_grid(n_rows), dim3(kBlock), 0, S(stream)>>>(indptr, indices, n_rows, a_dst, lda, b_src,
                                                                              ldb, sf, shift);
  });
  GTA_LAUNCHED("k_softmax_shift");
  return GTA_OK;
}

extern "C++" {  // C++ helpers (WavePlan is returned by value) inside the C ABI block
namespace {
// The operands of one UPDATE GEMM as the gta_update_mm* entries receive them (w: W for
// gta_update_mm, W^T for the _t forms).
struct MmArgs {
  const void* x;
  int64_t ldx;
  const int32_t* row_idx;
  int64_t M, K;
  const void* w;
  int64_t ldw, N;
  int dtype, sf;
  float* out;
  int64_t ldo;
};

// The checks of the three gta_update_mm* entries, in their order; sizes_ok / ptrs_ok carry what an
// entry adds to the size and pointer conditions.  GTA_OK with M == 0: nothing to do, and the
// pointers are not looked at.
int check_mm(const char* who, const MmArgs& a, bool sizes_ok = true, bool ptrs_ok = true) {
  const auto bad = [&](int code, const char* what) { return fail(code, std::string(who) + what); };
  if (a.M < 0 || a.K <= 0 || a.N <= 0 || !sizes_ok) return bad(GTA_ERR_ARG, ": bad sizes");
  if (a.M == 0) return GTA_OK;
  if (!a.x || !a.w || !a.out || !ptrs_ok) return bad(GTA_ERR_ARG, ": bad arguments");
  if (a.K > INT32_MAX || a.N > INT32_MAX) return bad(GTA_ERR_UNSUPPORTED, ": K/N too large");
  if (a.dtype != GTA_F32 && a.dtype != GTA_BF16 && a.dtype != GTA_F32_BF16) return bad(GTA_ERR_ARG, ": bad dtype");
  return GTA_OK;
}
}  // namespace
}  // extern "C++"

int gta_update_mm(const void* x, int64_t ldx, const int32_t* row_idx, int64_t M, int64_t K, const void* w,
                  int64_t ldw, int64_t N, int dtype, int sf, float* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  const MmArgs a{x, ldx, row_idx, M, K, w, ldw, N, dtype, sf, out, ldo};
  if (const int rc = check_mm("update_mm", a); rc != GTA_OK || M == 0) return rc;
  const dim3 grid(static_cast<unsigned>((M + 63) / 64), static_cast<unsigned>((N + 63) / 64));
  if (dtype == GTA_F32) {
    k_mm_f32<<<grid, dim3(kBlock), 0, S(stream)>>>(static_cast<const float*>(x), ldx, row_idx, M,
                                                   static_cast<int>(K), static_cast<const float*>(w), ldw,
                                                   static_cast<int>(N), sf, out, ldo);
  } else if (dtype == GTA_BF16) {
    k_mm_bf16<uint16_t><<<grid, dim3(kBlock), 0, S(stream)>>>(static_cast<const uint16_t*>(x), ldx, row_idx, M,
                                                              static_cast<int>(K), static_cast<const uint16_t*>(w),
                                                              ldw, static_cast<int>(N), sf, out, ldo);
  } else {
    k_mm_bf16<float><<<grid, dim3(kBlock), 0, S(stream)>>>(static_cast<const float*>(x), ldx, row_idx, M,
                                                           static_cast<int>(K), static_cast<const uint16_t*>(w), ldw,
                                                           static_cast<int>(N), sf, out, ldo);
  }
  GTA_LAUNCHED("k_mm");
  return GTA_OK;
}

extern "C++" {
namespace {
// waves per SIMD k_mm_wave<NT, FR> is built for (its __launch_bounds__): what its registers allow
constexpr int wave_wps(int NT, int FR) { return NT == 4 || FR <= 2 ? 2 : 1; }

// SIMDs of the current device (4 per CU: 1024 on an MI355X), read once per device (the
// grid cap and the cost model below follow the device, not a constant)
int64_t device_simds() {
  static std::atomic<int64_t> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1024;
  int64_t v = cache[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 1024;
  v = 4 * static_cast<int64_t>(cus);
  cache[dev].store(v, std::memory_order_relaxed);
  return v;
}

// k_mm_wave unit cost model, in FR = 4 units (64 rows) of one wave alone on a SIMD, per unit of
// each FR (profiles/r04/mm_wave_ab.log, K = 500 / 602): FR 3 (48 rows) 0.81, FR 2 (32 rows) 0.56 alone
// and 1.3 per pair sharing a SIMD (its 2-waves-per-SIMD build).  A launch takes as many rounds of
// its units as the most loaded SIMD holds: units spread over the device's SIMDs, FR 2 two deep.
double wave_cost(int fr, int64_t units, int64_t simds) {
  if (fr == 2) return units <= simds ? 0.56 : static_cast<double>((units + 2 * simds - 1) / (2 * simds)) * 1.3;
  return static_cast<double>((units + simds - 1) / simds) * (fr == 3 ? 0.81 : 1.0);
}

struct WavePlan {
  int fr = 4;          // FR of the first launch
  int64_t rows = 0;    // rows of the first launch (all of M when there is no second)
  int fr2 = 0;         // FR of the second launch over the remaining rows (0: none)
  double cost = 0.0;
};

// the cheapest single launch, or whole FR = 4 rounds (every SIMD the same number of units) and the
// remainder rows as a second launch with its own cheapest FR -- a partial last round of 64-row
// units leaves SIMDs idle (232,965 x 602: 3.56 rounds)
WavePlan wave_plan(int64_t M, int64_t ncb, int64_t simds) {
  WavePlan best;
  best.cost = 1e30;
  for (int f = 4; f >= 2; --f) {
    const double c = wave_cost(f, (M + 16 * f - 1) / (16 * f) * ncb, simds);
    if (c < best.cost - 1e-9) { best.cost = c; best.fr = f; best.rows = M; best.fr2 = 0; }
  }
  const int64_t rounds = M / 64 * ncb / simds;  // whole FR 4 rounds
  if (rounds >= 1) {
    const int64_t rows = rounds * simds / ncb * 64, rem = M - rows;
    if (rem > 0 && rows > 0) {
      for (int f = 4; f >= 2; --f) {
        const double c = static_cast<double>(rounds) + wave_cost(f, (rem + 16 * f - 1) / (16 * f) * ncb, simds) + 0.1;
        if (c < best.cost - 1e-9) { best.cost = c; best.fr = 4; best.rows = rows; best.fr2 = f; }
      }
    }
  }
  return best;
}

int64_t wave_units(int64_t M, int64_t ncb, int fr) { return (M + 16 * fr - 1) / (16 * fr) * ncb; }

// one k_mm_wave launch over rows [0, M) of x / out
void launch_wave_rows(int nt, int fr, hipStream_t s, const float* x, int64_t ldx, int64_t M, int K, const float* wt,
                      int64_t ldwt, int N, int sf, float* out, int64_t ldo) {
  const int64_t ncb = (N + 16 * nt - 1) / (16 * nt);
  const dim3 gr(static_cast<unsigned>(std::min<int64_t>(wave_units(M, ncb, fr), device_simds() * wave_wps(nt, fr))));
  const uint32_t xbu = static_cast<uint32_t>(((M - 1) * ldx + K) * 4);
  const uint32_t wbu = static_cast<uint32_t>((static_cast<int64_t>(N - 1) * ldwt + K) * 4);
#define GTA_WAVE(NT_, FR_) \
  k_mm_wave<NT_, FR_, wave_wps(NT_, FR_)><<<gr, dim3(kWave), 0, s>>>(x, ldx, M, K, wt, ldwt, N, sf, out, ldo, xbu, wbu)
  if (nt == 8) { if (fr == 2) GTA_WAVE(8, 2); else if (fr == 3) GTA_WAVE(8, 3); else GTA_WAVE(8, 4); }
  else { if (fr == 2) GTA_WAVE(4, 2); else if (fr == 3) GTA_WAVE(4, 3); else GTA_WAVE(4, 4); }
#undef GTA_WAVE
}

// k_mm_wave over the whole output when it is the better form (knob mm_wave: 0 never, 1 auto, 2
// whenever the shape allows; mm_wave_fr 2 / 3 / 4 forces one launch of that FR).  Auto: N > 64
// (NT = 8), K >= 256 and enough units to occupy most SIMDs; elsewhere k_mm_ring measured as fast
// or faster (profiles/r04/mm_wave_ab*.log).  Rows are independent, so the two-launch split is
// bitwise the one-launch result.  False: not taken (the caller runs k_mm_ring).
bool launch_wave(int nt, hipStream_t s, const float* x, int64_t ldx, int64_t M, int K, const float* wt, int64_t ldwt,
                 int N, int sf, float* out, int64_t ldo) {
  const int mode = tuning().mm_wave;
  const int64_t xb = ((M - 1) * ldx + K) * 4, wb = (static_cast<int64_t>(N - 1) * ldwt + K) * 4;
  if (mode == 0 || xb > 0xFFFFFFFFLL || wb > 0xFFFFFFFFLL || (nt != 4 && nt != 8) || K < 16) return false;
  const int64_t ncb = (N + 16 * nt - 1) / (16 * nt);
  const int frk = tuning().mm_wave_fr;
  WavePlan pl;
  if (frk == 2 || frk == 3 || frk == 4) {
    pl.fr = frk;
    pl.rows = M;
  } else {
    pl = wave_plan(M, ncb, device_simds());
  }
  if (mode == 1 && (nt != 8 || K < 256 || 4 * wave_units(pl.rows, ncb, pl.fr) < 3 * device_simds())) return false;
  launch_wave_rows(nt, pl.fr, s, x, ldx, pl.rows, K, wt, ldwt, N, sf, out, ldo);
  if (pl.fr2 && pl.rows < M)
    launch_wave_rows(nt, pl.fr2, s, x + pl.rows * ldx, ldx, M - pl.rows, K, wt, ldwt, N, sf, out + pl.rows * ldo, ldo);
  return true;
}

// k_mm_ring launch: NT (4: N <= 64, 8: wider), ring depth D (3: the persistent form, 4: split K),
// FR (A fragments per wave); kslice > 0: the split-K form (grid.y = K slices)
void launch_ring(int nt, int D, int fr, dim3 gr, hipStream_t s, const MmArgs& a, int kslice, int64_t slice_stride) {
#define GTA_RING(NT_, D_, FR_)                                                                                      \
  k_mm_ring<NT_, D_, FR_><<<gr, dim3(kBlock), 0, s>>>(static_cast<const float*>(a.x), a.ldx, a.row_idx, a.M,           \
                                                      static_cast<int>(a.K), static_cast<const float*>(a.w), a.ldw, \
                                                      static_cast<int>(a.N), a.sf, a.out, a.ldo, kslice, slice_stride)
#define GTA_RING_D(NT_, FR_) \
  if (D == 4) GTA_RING(NT_, 4, FR_); else GTA_RING(NT_, 3, FR_)
  if (nt == 8) { if (fr == 1) { GTA_RING_D(8, 1); } else { GTA_RING_D(8, 2); } }
  else { if (fr == 1) { GTA_RING_D(4, 1); } else { GTA_RING_D(4, 2); } }
#undef GTA_RING_D
#undef GTA_RING
}

// k_mm_rows launch: the TA / WT / NT / PF ladder (pf: prefetch the next A fragment); kslice > 0:
// the split-K form (grid.y = K slices, slice y into a.out + y * oslice)
void launch_rows(int dtype, int nt, bool pf, dim3 gr, hipStream_t s, const MmArgs& a, int64_t kslice, int64_t oslice) {
#define GTA_MMR(TA_, WT_, NT_, PF_)                                                                             \
  k_mm_rows<TA_, WT_, NT_, PF_><<<gr, dim3(kBlock), 0, s>>>(static_cast<const TA_*>(a.x), a.ldx, a.row_idx, a.M,     \
                                                            static_cast<int>(a.K), static_cast<const WT_*>(a.w),   \
                                                            a.ldw, static_cast<int>(a.N), a.sf, a.out, a.ldo,      \
                                                            kslice, oslice, 1)
#define GTA_MMR_PF(TA_, WT_, NT_) \
  if (pf) GTA_MMR(TA_, WT_, NT_, true); else GTA_MMR(TA_, WT_, NT_, false)
#define GTA_MMR_NT(TA_, WT_)                                                                            \
  if (nt == 1) { GTA_MMR_PF(TA_, WT_, 1); } else if (nt == 2) { GTA_MMR_PF(TA_, WT_, 2); }              \
  else if (nt == 4) { GTA_MMR_PF(TA_, WT_, 4); } else { GTA_MMR_PF(TA_, WT_, 8); }
  if (dtype == GTA_F32) { GTA_MMR_NT(float, float) }
  else if (dtype == GTA_BF16) { GTA_MMR_NT(uint16_t, uint16_t) }
  else { GTA_MMR_NT(float, uint16_t) }
#undef GTA_MMR_NT
#undef GTA_MMR_PF
#undef GTA_MMR
}

// CUs the persistent grids are sized for (an MI355X)
constexpr int64_t kMmCUs = 256;

// a persistent grid: per_cu blocks on every CU, whole column-block sets, at most one block per row group
inline int64_t persistent_blocks(int64_t n_grp, int64_t ncb, int64_t per_cu) {
  return std::min(n_grp, std::max<int64_t>(1, kMmCUs * per_cu / ncb)) * ncb;
}

// k_mm_rows prefetches the next A fragment: measured 1.2x on fp32 (K = 602) and bf16 K = 128, and 1.1x
// on the mixed path with a K tail since fp32 A loads are float4 pieces (GIN K = 100: 0.70 -> 0.64 ms,
// profiles/r01_mm_bench_2.json); bf16 x with a K tail (k: K, or the K slice) stays without;
// tuning().mm_prefetch 2 = always, 0 = never
inline bool rows_prefetch(int dtype, int64_t k) {
  return tuning().mm_prefetch == 2 || (tuning().mm_prefetch == 1 && (dtype != GTA_BF16 || k % 32 == 0));
}

inline int mm_nt(int64_t N) { return N <= 16 ? 1 : N <= 32 ? 2 : N <= 64 ? 4 : 8; }

// fp32 products the ring takes: 4-B aligned x rows (16-B DMA pieces at 4-B aligned addresses are
// fine), W^T rows 16-B aligned (ops._transposed pads them)
inline bool ring_ok(int dtype, int nt, const void* x, const void* wt, int64_t ldwt) {
  return tuning().mm_ring && dtype == GTA_F32 && nt >= 4 && aligned(x, 4) && aligned(wt, 16) && ldwt % 4 == 0;
}

// K slice of the split form: a multiple of 16 (whole ring stages; k_mm_rows masks a bf16 step's
// half past the slice end), the same for every kernel form so the forms stay bitwise equal
inline int64_t mm_kslice(int64_t K, int64_t splits) {
  const int64_t per = (K + splits - 1) / splits;
  return std::max<int64_t>(16, (per + 15) / 16 * 16);
}
}  // namespace
}  // extern "C++"

int64_t gta_update_mm_t_splits(int64_t M, int64_t K, int64_t N, int dtype, void* stream) {
  const CallTuning ct_(stream);  // the stream's attached knob set decides mm_split, as for the GEMM itself
  if (M < 0 || K <= 0 || N <= 0) return fail(GTA_ERR_ARG, "update_mm_t_splits: bad sizes");
  if (tuning().mm_split >= 0) return std::max<int64_t>(1, tuning().mm_split);
  const int nt = mm_nt(N);
  const int64_t units = (M + 127) / 128 * ((N + 16 * nt - 1) / (16 * nt));  // 128-row groups x column blocks
  if (K < 256 || units >= 128) return 1;
  // the ring (fp32): one (group, slice) block per CU, every block resident at once; k_mm_rows
  // (bf16 / mixed, several blocks per CU): about two per CU; slices of >= 64 k
  const int64_t want = (dtype == GTA_F32 ? kMmCUs : 2 * kMmCUs) / std::max<int64_t>(1, units);
  return std::max<int64_t>(1, std::min<int64_t>({want, K / 64, dtype == GTA_F32 ? 32 : 16}));
}

int gta_update_mm_t(const void* x, int64_t ldx, const int32_t* row_idx, int64_t M, int64_t K, const void* wt,
                    int64_t ldwt, int64_t N, int dtype, int sf, float* out, int64_t ldo, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  const MmArgs a{x, ldx, row_idx, M, K, wt, ldwt, N, dtype, sf, out, ldo};
  if (const int rc = check_mm("update_mm_t", a, ldwt >= K); rc != GTA_OK || M == 0) return rc;
  const int nt = mm_nt(N);
  const int64_t groups = (M + 127) / 128;
  const int64_t ncb = (N + 16 * nt - 1) / (16 * nt);
  // (mm_ring = 0 selects k_mm_rows, and a forced ring shape (mm_ring_fr) the ring)
  if (dtype == GTA_F32 && tuning().mm_wave && tuning().mm_ring && !tuning().mm_ring_fr && !row_idx && K >= 16 &&
      launch_wave(nt, S(stream), static_cast<const float*>(x), ldx, M, static_cast<int>(K), static_cast<const float*>(wt),
                  ldwt, static_cast<int>(N), sf, out, ldo)) {
    GTA_LAUNCHED("k_mm_wave");
    return GTA_OK;
  }
  if (K >= 32 && ring_ok(dtype, nt, x, wt, ldwt)) {
    // 64-row groups (one A fragment per wave, twice the work units for the per-CU balance) when
    // 128-row groups load the CUs unevenly on a short K, where per-group start-up and epilogue weigh
    // most, or when there are too few 128-row groups for two blocks per CU (K = 128 / 256 at 232,965
    // rows 77 -> 86 / 92 -> 96 TF/s, 16,384 rows 40 -> 69; profiles/r02_mm_ring_probe_fr.json)
    const int frk = tuning().mm_ring_fr;
    const double per_cu2 = static_cast<double>(groups * ncb) / static_cast<double>(kMmCUs);
    const bool uneven = per_cu2 / std::ceil(per_cu2) < 0.95;
    const int fr = (frk == 1 || (frk == 0 && ((K <= 256 && uneven) || groups < 512))) ? 1 : 2;
    const int64_t n_grp = fr == 1 ? (M + 63) / 64 : groups;
    // the persistent 3-deep ring with every CU slot its LDS allows filled (each CU the same number of
    // row groups +-1; profiles/r02_mm_ring_probe.json); 4 or 8 stages at fewer blocks per CU were
    // measured slower on every shape from 16,384 to 232,965 rows (profiles/r03/mm_depth_sweep.log)
    const int64_t blocks = persistent_blocks(n_grp, ncb, ring_blocks(nt, 3, fr));
    launch_ring(nt, 3, fr, dim3(static_cast<unsigned>(blocks)), S(stream), a, 0, 0);
    GTA_LAUNCHED("k_mm_ring");
    return GTA_OK;
  }
  if (dtype != GTA_F32 && tuning().mm_ring && nt >= 4 && K <= 256 &&
      (dtype == GTA_F32_BF16 ? aligned(x, 4) : (aligned(x, 16) && ldx % 8 == 0))) {
    // bf16 MFMA with the x ring (fp32 x: 64-row groups, 6 stages, two blocks per CU; bf16 x: the
    // same stages hold twice the k) and W^T resident in LDS; mm_ring_fr = 2: 128-row groups, 3 stages
    const int fr = tuning().mm_ring_fr == 2 ? 2 : 1;
    const int sb = K <= 128 ? 4 : 8;
    const int64_t n_grp = fr == 1 ? (M + 63) / 64 : groups;
    const dim3 gr(static_cast<unsigned>(persistent_blocks(n_grp, ncb, 2)));
#define GTA_RBF(TA_, NT_, D_, FR_, SB_)                                                                        \
  k_mm_ring_bf<TA_, NT_, D_, FR_, SB_><<<gr, dim3(kBlock), 0, S(stream)>>>(static_cast<const TA_*>(x), ldx, row_idx, M, \
                                                                          static_cast<int>(K),                       \
                                                                          static_cast<const uint16_t*>(wt), ldwt,    \
                                                                          static_cast<int>(N), sf, out, ldo)
#define GTA_RBF_F(TA_, NT_, SB_) \
  if (fr == 2) GTA_RBF(TA_, NT_, 3, 2, SB_); else GTA_RBF(TA_, NT_, 6, 1, SB_)
#define GTA_RBF_S(TA_, NT_) if (sb == 4) { GTA_RBF_F(TA_, NT_, 4); } else { GTA_RBF_F(TA_, NT_, 8); }
    if (dtype == GTA_F32_BF16) { if (nt == 8) { GTA_RBF_S(float, 8); } else { GTA_RBF_S(float, 4); } }
    else { if (nt == 8) { GTA_RBF_S(uint16_t, 8); } else { GTA_RBF_S(uint16_t, 4); } }
#undef GTA_RBF_S
#undef GTA_RBF_F
#undef GTA_RBF
    GTA_LAUNCHED("k_mm_ring_bf");
    return GTA_OK;
  }
  const int kc = (dtype == GTA_F32) ? (nt >= 8 ? 64 : 128) : (nt >= 8 ? 128 : 256);  // k_mm_rows KC
  const int64_t blocks = K <= kc ? persistent_blocks(groups, ncb, 8) : groups * ncb;  // W staged once: persistent
  launch_rows(dtype, nt, rows_prefetch(dtype, K), dim3(static_cast<unsigned>(blocks)), S(stream), a, 0, 0);
  GTA_LAUNCHED("k_mm_rows");
  return GTA_OK;
}

int gta_update_mlp(const void* x, int64_t ldx, int64_t M, int64_t K1, const void* w1t, int64_t ldw1, int64_t N1,
                   int sf1, const void* w2t, int64_t ldw2, int64_t N2, int sf2, int dtype, float* out, int64_t ldo,
                   void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (M < 0 || K1 <= 0 || N1 <= 0 || N2 <= 0 || ldw1 < K1 || ldw2 < N1 || ldx < K1 || ldo < N2)
    return fail(GTA_ERR_ARG, "update_mlp: bad sizes");
  if (M == 0) return GTA_OK;
  if (!x || !w1t || !w2t || !out) return fail(GTA_ERR_ARG, "update_mlp: bad arguments");
  if (dtype != GTA_F32_BF16 && dtype != GTA_BF16)
    return fail(GTA_ERR_UNSUPPORTED, "update_mlp: fp32 or bf16 x with bf16 weights only");
  if (K1 > 128 || N1 > 128 || N2 > 128) return fail(GTA_ERR_UNSUPPORTED, "update_mlp: K1, N1, N2 <= 128");
  const bool xb = dtype == GTA_BF16;
  if (K1 % 4 || ldx % (xb ? 8 : 4) || !aligned(x, 16) || ldx > (1 << 20))
    return fail(GTA_ERR_UNSUPPORTED, "update_mlp: x rows 16-B aligned with K1 % 4 == 0");
  const int64_t n_groups = (M + 15) / 16;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n_groups + kWavesPerBlock - 1) / kWavesPerBlock, 512));
  const dim3 gr(static_cast<unsigned>(blocks));
  const uint16_t* w1 = static_cast<const uint16_t*>(w1t);
  const uint16_t* w2 = static_cast<const uint16_t*>(w2t);
  const int k1 = static_cast<int>(K1), n1 = static_cast<int>(N1), n2 = static_cast<int>(N2);
  const bool c1 = sf1 == GTA_SF_NONE || sf1 == GTA_SF_RELU, c2 = sf2 == GTA_SF_NONE || sf2 == GTA_SF_RELU;
#define GTA_MLP(A_, B_)                                                                                          \
  do {                                                                                                           \
    if (xb) k_mlp_bf<A_, B_, uint16_t><<<gr, dim3(kBlock), 0, S(stream)>>>(static_cast<const uint16_t*>(x), ldx, M,  \
                                                                        k1, w1, ldw1, n1, sf1, w2, ldw2, n2, sf2, \
                                                                        out, ldo);                                \
    else k_mlp_bf<A_, B_, float><<<gr, dim3(kBlock), 0, S(stream)>>>(static_cast<const float*>(x), ldx, M, k1, w1,    \
                                                                     ldw1, n1, sf1, w2, ldw2, n2, sf2, out, ldo); \
  } while (0)
  if (c1 && c2) {
    if (sf1 == GTA_SF_RELU) { if (sf2 == GTA_SF_RELU) GTA_MLP(GTA_SF_RELU, GTA_SF_RELU); else GTA_MLP(GTA_SF_RELU, GTA_SF_NONE); }
    else { if (sf2 == GTA_SF_RELU) GTA_MLP(GTA_SF_NONE, GTA_SF_RELU); else GTA_MLP(GTA_SF_NONE, GTA_SF_NONE); }
  } else {
    GTA_MLP(-1, -1);
  }
#undef GTA_MLP
  GTA_LAUNCHED("k_mlp_bf");
  return GTA_OK;
}

int64_t gta_update_mm_t_split_workspace_bytes(int64_t M, int64_t K, int64_t N, int64_t splits) {
  if (M < 0 || K <= 0 || N <= 0 || splits < 1) return fail(GTA_ERR_ARG, "update_mm_t_split_workspace_bytes: bad sizes");
  return splits * M * N * static_cast<int64_t>(sizeof(float));  // every slice rounding gives <= splits slices
}

int gta_update_mm_t_split(const void* x, int64_t ldx, const int32_t* row_idx, int64_t M, int64_t K, const void* wt,
                          int64_t ldwt, int64_t N, int dtype, int sf, float* out, int64_t ldo, int64_t splits,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  const MmArgs a{x, ldx, row_idx, M, K, wt, ldwt, N, dtype, sf, out, ldo};
  if (const int rc = check_mm("update_mm_t_split", a, ldwt >= K && splits >= 1, workspace != nullptr);
      rc != GTA_OK || M == 0)
    return rc;
  if (workspace_bytes < splits * M * N * static_cast<int64_t>(sizeof(float)))
    return fail(GTA_ERR_ARG, "update_mm_t_split: workspace too small");
  float* ws = static_cast<float*>(workspace);
  const int nt = mm_nt(N);
  const int64_t groups = (M + 127) / 128;
  const int64_t ncb = (N + 16 * nt - 1) / (16 * nt);
  hipStream_t s = S(stream);
  const bool ring = ring_ok(dtype, nt, x, wt, ldwt) && N % 4 == 0 && aligned(ws, 16);
  const int64_t ks = mm_kslice(K, splits), nsl = (K + ks - 1) / ks;
  if (nsl > 65535) return fail(GTA_ERR_UNSUPPORTED, "update_mm_t_split: too many slices");
  MmArgs part = a;  // the slices: dense [M, N] partial sums in the workspace, no SF
  part.out = ws;
  part.ldo = N;
  if (ring) {
    // every (64-row group, K slice) on its own block, a 4-deep ring at three blocks per CU, then the
    // ordered slice sum.  GCN Cora's [2708 x 1433].[1433 x 128]: 43 groups x 10 slices of 144 k,
    // 28.8 us against 31.5 for 128-row groups on an 8-deep ring at one block per CU
    // (profiles/r03/mm_cora_epilogue.log); mm_ring_fr = 2 selects 128-row groups
    const int fr = tuning().mm_ring_fr == 2 ? 2 : 1;
    const int64_t n_grp = fr == 1 ? (M + 63) / 64 : groups;
    part.sf = GTA_SF_NONE;
    launch_ring(nt, 4, fr, dim3(static_cast<unsigned>(n_grp * ncb), static_cast<unsigned>(nsl)), s, part,
                static_cast<int>(ks), M * N);
    GTA_LAUNCHED("k_mm_ring<split>");
  } else {
    launch_rows(dtype, nt, rows_prefetch(dtype, ks), dim3(static_cast<unsigned>(groups * ncb), static_cast<unsigned>(nsl)),
                s, part, ks, M * N);
    GTA_LAUNCHED("k_mm_rows<split>");
  }
  const int64_t total = M * N;
  if (N % 4 == 0 && ldo % 4 == 0 && aligned(out, 16) && aligned(ws, 16)) {
    const int64_t t4 = total / 4;
    k_mm_slices_sum4<<<dim3(static_cast<unsigned>(std::min<int64_t>((t4 + kBlock - 1) / kBlock, 4096))), dim3(kBlock), 0,
                       s>>>(reinterpret_cast<const float4*>(ws), static_cast<int>(nsl), M, static_cast<int>(N / 4), sf,
                            out, ldo);
  } else {
    k_mm_slices_sum<<<dim3(static_cast<unsigned>(std::min<int64_t>((total + kBlock - 1) / kBlock, 4096))), dim3(kBlock), 0,
                      s>>>(ws, static_cast<int>(nsl), M, static_cast<int>(N), sf, out, ldo);
  }
  GTA_LAUNCHED("k_mm_slices_sum");
  return GTA_OK;
}

int gta_tile_nnz(const int64_t* indptr, const int32_t* indices, int64_t n_rows, int64_t n_cols, int64_t T,
                 int32_t* counts, void* stream) {
  const CallTuning ct_(stream);  // knobs attached to this stream, if any (gta_tuning_attach)
  if (!indptr || !counts || n_rows < 0 || n_cols <= 0 || T <= 0)
    return fail(GTA_ERR_ARG, "tile_nnz: bad arguments");
  if (n_rows == 0) return GTA_OK;
  const dim3 grid = row_grid(n_rows);
  k_tile_nnz<<<grid, dim3(kBlock), 0, S(stream)>>>(indptr, indices, n_rows, n_cols, T, counts);
  GTA_LAUNCHED("k_tile_nnz");
  return GTA_OK;
}

int gta_synth_alpha(const int64_t* indptr, const int64_t* gen, int64_t n_rows, int64_t nnz, int heads, int64_t seed,
                    int64_t logit_stream, float* out, void* stream) {
  if (!indptr || n_rows < 0 || nnz < 0 || heads <= 0 || heads > kWave || kWave % heads != 0 || seed < 0 ||
      logit_stream < 0 || (nnz > 0 && (!gen || !out)))
    return fail(GTA_ERR_ARG, "synth_alpha: bad arguments (heads must divide 64)");
  if (n_rows == 0 || nnz == 0) return GTA_OK;
  const uint32_t s1 = static_cast<uint32_t>(2 * logit_stream), s2 = s1 + 1u;
  const dim3 grid = row_grid(n_rows);
  k_synth_alpha<<<grid, dim3(kBlock), 0, S(stream)>>>(indptr, gen, n_rows, heads, mix32(hash_key(seed, s1)), s1,
                                                     mix32(hash_key(seed, s2)), s2, out);
  GTA_LAUNCHED("k_synth_alpha");
  return GTA_OK;
}

int gta_row_ids(const int64_t* indptr, int64_t n_rows, int64_t nnz, int64_t* out, void* stream) {
  if (!indptr || n_rows < 0 || nnz < 0 || (nnz > 0 && !out)) return fail(GTA_ERR_ARG, "row_ids: bad arguments");
  if (n_rows == 0 || nnz == 0) return GTA_OK;
  const dim3 grid = row_grid(n_rows);
  k_row_ids<<<grid, dim3(kBlock), 0, S(stream)>>>(indptr, n_rows, out);
  GTA_LAUNCHED("k_row_ids");
  return GTA_OK;
}

// _build.py passes a hash of this file and include/gta.h; _lib.load() refuses a library whose id
// differs from the sources beside it (a stale binary never runs silently)
#ifndef GTA_BUILD_ID
#define GTA_BUILD_ID "unversioned"
#endif
const char* gta_build_id(void) { return GTA_BUILD_ID; }

}  // extern "C"
