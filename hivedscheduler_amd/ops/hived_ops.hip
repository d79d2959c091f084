// MI355X (gfx950) GPU health-probe kernels.
//
// The scheduler grounds cell healthiness in measured hardware facts (the
// reference trusts K8s NodeReady only). These kernels give
// per-GPU signals that feed leaf-cell health:
//  - hbm_triad:  streaming HBM3E bandwidth (expected ~6 TB/s class; a sick
//                stack shows up as a large deficit)
//  - mfma_check: bf16 MFMA tile GEMM on every CU; the host compares every
//                wave's tile with the exact float64 product of operands built
//                so that fp32 holds it exactly — catches broken matrix cores
//  - mfma_burn:  sustained, timed MFMA issue per datapath, verified bitwise in
//                the kernel; TFLOP/s plus the CU of any wave that was wrong
//  - mx_scale_tile / mx_scale_burn: the block-scaled MFMA with per-lane E8M0
//                scales, all four scale bytes, e5m2 and the 6-bit formats, mixed
//                formats and the 32x32x64 shape, bitwise against float64
//  - matrix_tile / matrix_burn: the f64, f32, f16, i8, e5m2 and 32x32 MFMA
//                shapes and the 2:4 sparse smfmac forms, bitwise against float64
//                or int64; the CU of any wave whose burn was wrong
//  - lds_march:  all 160 KiB of every CU's LDS, both bit polarities, narrow
//                and wide reads, timed; the CU, word and bits of any mismatch
//  - valu_burn:  sustained, timed vector-ALU issue per section (integer, f32,
//                f64, cross-lane, transcendental), verified bitwise in the
//                kernel; the SIMD of any wave that was wrong
//  - vgpr_march: 480 of the 512 vector registers per lane of every SIMD, both
//                bit polarities; the SIMD, register and bits of any mismatch
//  - salu_burn:  sustained, timed scalar-ALU issue per section (32-bit, 64-bit,
//                SCC and control flow, EXEC masks), verified bitwise in the
//                kernel; the SIMD of any wave that was wrong
//  - sgpr_march: s32..s101 of every wave, both bit polarities, values unique
//                across waves; the SIMD, register and bits of any mismatch
//  - scalar_load_check: a pattern and its complement read through the scalar
//                data cache in all five load widths, compared on the SALU
//  - atomic_burn: global and LDS atomics (integer, float, packed, cmpswap) on
//                cells each lane owns, returning and non-returning, every
//                returned value and final cell verified bitwise; the CU of any
//                wave that was wrong
//  - atomic_contend: tickets, order-independent reductions and a cmpswap loop
//                from every workgroup on a few shared cells, judged by the host
//  - hbm_march:  a bounded span of HBM, both bit polarities, 16 B per lane,
//                values unique across the sweep; the offset, bits and direction
//                of any mismatch, and a bandwidth per XCD from device clocks
//  - mempath_probe: buffer loads and stores in every width, the descriptor's
//                bounds check at sharp lengths, direct-to-LDS loads and the
//                sub-dword, d16 and wide forms, every value verified bitwise;
//                the CU and instruction form of any mismatch
//  - cvt_sweep / cvt_burn: the fp8 / fp6 / fp4 / bf16 conversion instructions,
//                scaled, unscaled and stochastic rounding, every select, bitwise
//                against a host mirror; the SIMD of any wave that was wrong
//  - lds_tr_read / gemm_pipe: the LDS transpose reads as data movement, and a
//                tiled bf16 / fp8 GEMM (direct-to-LDS loads in flight, LDS
//                fragment reads and MFMAs in the same cycles), exact and
//                compared bitwise in registers; the CU of any wave that was wrong
//  - mx_gemm_pipe: the same pipeline through the block-scaled MFMA: a tiled
//                MXFP8 / MXFP4 GEMM whose E8M0 scale bytes are streamed from
//                memory beside the operands, exact and compared bitwise
//  - mx6_gemm_pipe: that pipeline for rows that are not 128 bytes: MXFP6 / MXBF6
//                (96-byte rows, ds_read_b96_tr_b6 for B kn) and an MXFP8 A against
//                MXFP6 / MXFP4 weights, exact and compared bitwise
//  - p2p copy:  xGMI link bandwidth between two GPUs (expected ~153 GB/s per
//                link per direction); a degraded link marks the PAIR cell bad
//
// Written CDNA4-native: 64-wide wavefronts, float4 coalesced loads,
// __builtin_amdgcn_mfma_f32_16x16x32_bf16 per-wave tiles.
//
// What the probes share is defined once, right below: host guards and event
// timing (EventPair, DeviceAllocs, OwnedStream, timed_ms, warm_then_timed_ms,
// zero_records, dispatch_int), device helpers (hw_word, wave_*, store_record8).
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#define HIP_CHECK(cmd)                                                                     \
  do {                                                                                     \
    hipError_t hip_check_e = (cmd); /* a name no argument uses */                          \
    TORCH_CHECK(hip_check_e == hipSuccess, "HIP error: ", hipGetErrorString(hip_check_e),  \
                " at ", __FILE__, ":", __LINE__);                                          \
  } while (0)

// ---------------------------------------------------------------------------
// Host scaffolding. The agent calls the entry points every round in a
// long-lived process on a GPU that may be failing, so a guard owns whatever
// they create: a check that throws leaves no event, stream or allocation behind.
// ---------------------------------------------------------------------------
// a start/stop event pair
struct EventPair {
  hipEvent_t start = nullptr, stop = nullptr;
  EventPair() {
    HIP_CHECK(hipEventCreate(&start));
    hipError_t e = hipEventCreate(&stop);
    if (e != hipSuccess) (void)hipEventDestroy(start);  // no destructor will run
    HIP_CHECK(e);
  }
  ~EventPair() {
    (void)hipEventDestroy(start);
    (void)hipEventDestroy(stop);
  }
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
};

// Device allocations from plain hipMalloc, freed on scope exit. free_all() is
// the checked release of the success path, in allocation order; what a failed
// hipFree leaves in the list, the destructor still tries.
struct DeviceAllocs {
  std::vector<void*> ptrs;
  DeviceAllocs() = default;
  ~DeviceAllocs() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  DeviceAllocs(const DeviceAllocs&) = delete;
  DeviceAllocs& operator=(const DeviceAllocs&) = delete;
  // !required: nullptr, and no error left pending, when no such block is left
  void* alloc(size_t bytes, bool required = true) {
    ptrs.reserve(ptrs.size() + 1);  // the push_back below cannot throw
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess && !required) {
      (void)hipGetLastError();
      return nullptr;
    }
    HIP_CHECK(e);
    ptrs.push_back(p);
    return p;
  }
  void* alloc_zeroed(size_t bytes) {
    void* p = alloc(bytes);
    HIP_CHECK(hipMemset(p, 0, bytes));
    return p;
  }
  void free_all() {
    while (!ptrs.empty()) {
      void* p = ptrs.front();
      ptrs.erase(ptrs.begin());
      HIP_CHECK(hipFree(p));
    }
  }
};

// a stream of our own (the p2p copy must not queue behind torch's work)
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() { HIP_CHECK(hipStreamCreate(&s)); }
  ~OwnedStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  void destroy() {
    hipStream_t mine = s;
    s = nullptr;
    HIP_CHECK(hipStreamDestroy(mine));
  }
};

// Milliseconds that what `launch` enqueues on `stream` takes, between two
// events. The torch stream is non-blocking: a legacy-stream hipMemcpy does not
// order against it, so nothing may read what the launch wrote, or the timing,
// before the stop event has been waited for. That wait is in here.
template <typename F>
static double timed_ms(hipStream_t stream, F&& launch) {
  EventPair ev;
  HIP_CHECK(hipEventRecord(ev.start, stream));
  launch();
  HIP_CHECK(hipEventRecord(ev.stop, stream));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventSynchronize(ev.stop));
  float ms = 0;
  HIP_CHECK(hipEventElapsedTime(&ms, ev.start, ev.stop));
  return (double)ms;
}

// one untimed warm-up launch (code-object load and clock ramp stay out of the
// timing), then one timed launch
template <typename F>
static double warm_then_timed_ms(hipStream_t stream, F&& launch) {
  launch();
  HIP_CHECK(hipGetLastError());
  return timed_ms(stream, launch);
}

// the zeroed int32 [waves, width] tensor the per-wave records land in
static torch::Tensor zero_records(long waves, long width, torch::Device device = torch::kCUDA) {
  return torch::zeros({waves, width}, torch::TensorOptions().dtype(torch::kInt32).device(device));
}

// f(std::integral_constant<int, I>{}) for the I in [0, N) that equals `value`:
// a runtime enum becomes the template argument of a kernel
template <int N, typename F>
static void dispatch_int(int value, F&& f) {
  if constexpr (N > 1) {
    if (value != N - 1) return dispatch_int<N - 1>(value, f);
  }
  f(std::integral_constant<int, N - 1>{});
}

// ---------------------------------------------------------------------------
// Device scaffolding.
//
// Placement word: where a wave runs, for the host to join a result to the
// hardware that produced it (ops.decode_hw_word / decode_hw_simd). HW_ID
// (gfx9-family layout): SIMD_ID[5:4], CU_ID[11:8], SH_ID[12], SE_ID[15:13];
// XCC_ID identifies the XCD (0-7). The word is (XCC_ID << 16) | HW_ID[15:0].
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned hw_word() {
  unsigned hwid, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return (xcc << 16) | (hwid & 0xffff);
}

// Wave reductions with xor-butterfly shuffles: every lane ends up with the
// result over all 64 lanes. T is unsigned (one shuffle per step) or unsigned
// long long (two, one per half). They use no LDS of the workgroup's own.
// Users: the burn-in's checksum and the HBM march's verify kernel. The
// reductions of lds_march_kernel, valu_burn_kernel and vgpr_march_kernel, and
// the one in the burn-in's round loop, stay written out on __shfl_xor: through
// these (or lane_xor alone) the compiler allocates registers differently in
// those kernels' timed loops (BENCHMARKS.md "Probe scaffolding").
__device__ __forceinline__ unsigned lane_xor(unsigned v, int off) {
  return (unsigned)__shfl_xor((int)v, off);
}
__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int off) {
  int lo = __shfl_xor((int)(unsigned)v, off);
  int hi = __shfl_xor((int)(unsigned)(v >> 32), off);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
template <typename T> __device__ __forceinline__ T wave_add(T v) {
  for (int off = 32; off > 0; off >>= 1) v += lane_xor(v, off);
  return v;
}
template <typename T> __device__ __forceinline__ T wave_or(T v) {
  for (int off = 32; off > 0; off >>= 1) v |= lane_xor(v, off);
  return v;
}
template <typename T> __device__ __forceinline__ T wave_xor(T v) {
  for (int off = 32; off > 0; off >>= 1) v ^= lane_xor(v, off);
  return v;
}
template <typename T> __device__ __forceinline__ T wave_min(T v) {
  for (int off = 32; off > 0; off >>= 1) v = min(v, lane_xor(v, off));
  return v;
}

// a per-wave record of eight int32 leaves as two int4 vector stores
__device__ __forceinline__ void store_record8(int4* __restrict__ records, int wave, int r0, int r1,
                                              int r2, int r3, int r4, int r5, int r6, int r7) {
  records[2 * wave] = make_int4(r0, r1, r2, r3);
  records[2 * wave + 1] = make_int4(r4, r5, r6, r7);
}

// ---------------------------------------------------------------------------
// HBM streaming bandwidth: c = a + 2*b (triad), float4 per lane.
// ---------------------------------------------------------------------------
__global__ void triad_kernel(const float4* __restrict__ a, const float4* __restrict__ b,
                             float4* __restrict__ c, long n) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float4 av = a[i];
    float4 bv = b[i];
    float4 cv;
    cv.x = av.x + 2.0f * bv.x;
    cv.y = av.y + 2.0f * bv.y;
    cv.z = av.z + 2.0f * bv.z;
    cv.w = av.w + 2.0f * bv.w;
    c[i] = cv;
  }
}

// Returns achieved GB/s (3 streams: 2 reads + 1 write).
double hbm_triad_gbps(long size_mb, long iters, long blocks, long threads) {
  TORCH_CHECK(size_mb > 0 && iters > 0 && blocks > 0 && threads > 0 && threads <= 1024);
  long bytes = size_mb * 1024 * 1024;
  long n = bytes / sizeof(float4);
  auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA);
  auto a = torch::ones({bytes / 4}, opts);
  auto b = torch::ones({bytes / 4}, opts);
  auto c = torch::empty({bytes / 4}, opts);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&]() {
    hipLaunchKernelGGL(triad_kernel, dim3(blocks), dim3(threads), 0, stream,
                       reinterpret_cast<const float4*>(a.data_ptr<float>()),
                       reinterpret_cast<const float4*>(b.data_ptr<float>()),
                       reinterpret_cast<float4*>(c.data_ptr<float>()), n);
  };
  launch();  // warm-up, untimed
  const double ms = timed_ms(stream, [&]() {
    for (long it = 0; it < iters; it++) launch();
  });
  double sec = ms / 1e3;
  return (3.0 * bytes * iters) / sec / 1e9;
}

// ---------------------------------------------------------------------------
// MFMA health check: every wave computes the same 16x16 = (16x32)x(32x16)
// bf16 tile with v_mfma_f32_16x16x32_bf16 and writes its result. The host
// (ops/mfma_tiles.py) builds operands whose product fp32 holds exactly in any
// summation order and requires every wave's tile to equal it: no tolerance.
// Grid >> 256 CUs so every CU's matrix pipes execute it.
//
// Fragment layout (gfx950, 16x16x32 bf16):
//   A: lane l holds A[m = l&15][k = (l>>4)*8 + j], j in [0,8)
//   B: lane l holds B[k = (l>>4)*8 + j][n = l&15]
//   C/D: lane l reg r -> C[row = (l>>4)*4 + r][col = l&15]
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) short frag8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// the [waves, 16, 16] fp32 tiles the single-tile checks return
static torch::Tensor tile_output(long waves, torch::Device device) {
  return torch::empty({waves, 16, 16},
                      torch::TensorOptions().dtype(torch::kFloat32).device(device));
}

__global__ void mfma_check_kernel(const short* __restrict__ A, const short* __restrict__ B,
                                  float* __restrict__ C, int repeats) {
  int lane = threadIdx.x & 63;
  int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int m = lane & 15;
  int kbase = (lane >> 4) * 8;
  frag8 a, b;
  for (int j = 0; j < 8; j++) {
    a[j] = A[m * 32 + kbase + j];
    b[j] = B[(kbase + j) * 16 + m];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < repeats; r++) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, t, 0, 0, 0);
    acc = t;
  }
  float* out = C + (size_t)wave * 256;
  for (int r = 0; r < 4; r++) {
    int row = (lane >> 4) * 4 + r;
    out[row * 16 + m] = acc[r];
  }
}

// A: [16,32] bf16, B: [32,16] bf16 -> returns [waves, 16, 16] fp32 tiles.
torch::Tensor mfma_check(torch::Tensor A, torch::Tensor B, long blocks, long repeats) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "A/B must be on GPU");
  TORCH_CHECK(A.dtype() == torch::kBFloat16 && B.dtype() == torch::kBFloat16);
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
              B.sizes() == torch::IntArrayRef({32, 16}));
  A = A.contiguous();
  B = B.contiguous();
  int threads = 256;
  auto C = tile_output(blocks * (threads / 64), A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mfma_check_kernel, dim3(blocks), dim3(threads), 0, stream,
                     reinterpret_cast<const short*>(A.data_ptr()),
                     reinterpret_cast<const short*>(B.data_ptr()), C.data_ptr<float>(),
                     (int)repeats);
  HIP_CHECK(hipGetLastError());
  return C;
}

// ---------------------------------------------------------------------------
// FP8 MFMA health check (CDNA4 low-precision pipes). MI355X's headline
// compute is FP8/FP6/FP4; a GPU whose bf16 matrix pipes work but whose fp8
// datapath is broken would pass the bf16 check above. Same tile protocol as
// mfma_check: every wave computes one 16x16 = (16x32 @ 32x16) tile with
// v_mfma_f32_16x16x32_fp8_fp8 (OCP e4m3). The host requires every wave's tile
// to equal the float64 product of the decoded bytes (ops/mfma_tiles.py). The
// pipe is narrower than fp32 inside one 16-lane group's share of K (measured:
// a product more than 13 bits below the group's largest loses its low bits),
// so the host's operands put one exponent field in each row of A and each
// column of B: all products of an output element then share one power of two.
//
// Fragment layout mirrors the bf16 16x16x32 shape (8 K-elements per lane,
// here 8 fp8 bytes packed into one i64): lane l holds
// A[m=l&15][k=(l>>4)*8+j] and B[k=(l>>4)*8+j][n=l&15], j in [0,8);
// C/D layout is dtype-independent on gfx950.
// ---------------------------------------------------------------------------
__global__ void mfma_check_fp8_kernel(const unsigned char* __restrict__ A,
                                      const unsigned char* __restrict__ B,
                                      float* __restrict__ C) {
  int lane = threadIdx.x & 63;
  int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int m = lane & 15;
  int kbase = (lane >> 4) * 8;
  long a = 0, b = 0;
  for (int j = 0; j < 8; j++) {
    a |= (long)A[m * 32 + kbase + j] << (8 * j);
    b |= (long)B[(kbase + j) * 16 + m] << (8 * j);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, acc, 0, 0, 0);
  float* out = C + (size_t)wave * 256;
  for (int r = 0; r < 4; r++) {
    int row = (lane >> 4) * 4 + r;
    out[row * 16 + m] = acc[r];
  }
}

// A: [16,32] uint8 (raw OCP e4m3 bytes), B: [32,16] uint8
// -> [waves, 16, 16] fp32 tiles.
torch::Tensor mfma_check_fp8(torch::Tensor A, torch::Tensor B, long blocks) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "A/B must be on GPU");
  TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8,
              "A/B must be uint8 (raw fp8 e4m3 bytes)");
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 32}) &&
              B.sizes() == torch::IntArrayRef({32, 16}));
  A = A.contiguous();
  B = B.contiguous();
  int threads = 256;
  auto C = tile_output(blocks * (threads / 64), A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mfma_check_fp8_kernel, dim3(blocks), dim3(threads), 0, stream,
                     A.data_ptr<unsigned char>(), B.data_ptr<unsigned char>(),
                     C.data_ptr<float>());
  HIP_CHECK(hipGetLastError());
  return C;
}

// ---------------------------------------------------------------------------
// MX block-scaled MFMA health check: v_mfma_f32_16x16x128_f8f6f4, the
// gfx950-only instruction behind the FP8 (~5 PF) and FP4 (~10 PF) headline
// rates. fmt selects A/B element format: 0=fp8(e4m3), 4=fp4(e2m1).
// K=128: lane l holds A[m=l&15][k=(l>>4)*32+j], j in [0,32) — 32 bytes
// (8 VGPRs) for fp8; for fp4, 32 elements packed 2-per-byte into 16 bytes
// (low nibble = even k). Scales are e8m0 (2^(s-127)), one byte for A and one
// for B, broadcast to all four byte positions of every lane's scale operand:
// a uniform scale multiplies the tile by 2^(sa+sb-254) whatever the scale
// select and lane mapping are. 0x7F7F7F7F = 1.0 gives the plain product. The
// host verifies every tile against the exact product, as for the other checks.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) int i32x8;

template <int fmt>  // immediate operand: FMT must be a compile-time constant
__global__ void mfma_check_mx_kernel(const unsigned char* __restrict__ A,
                                     const unsigned char* __restrict__ B,
                                     float* __restrict__ C, int scale_a, int scale_b) {
  int lane = threadIdx.x & 63;
  int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int m = lane & 15;
  int kbase = (lane >> 4) * 32;
  union { i32x8 v; unsigned char b[32]; } a, b;
  a.v = (i32x8){0, 0, 0, 0, 0, 0, 0, 0};
  b.v = a.v;
  if constexpr (fmt == 0) {  // fp8: one byte per element
    for (int j = 0; j < 32; j++) {
      a.b[j] = A[m * 128 + kbase + j];
      b.b[j] = B[(kbase + j) * 16 + m];
    }
  } else {  // fp4: two elements per byte, low nibble first
    for (int j = 0; j < 32; j += 2) {
      unsigned lo = A[m * 128 + kbase + j] & 0xF;
      unsigned hi = A[m * 128 + kbase + j + 1] & 0xF;
      a.b[j / 2] = lo | (hi << 4);
      lo = B[(kbase + j) * 16 + m] & 0xF;
      hi = B[(kbase + j + 1) * 16 + m] & 0xF;
      b.b[j / 2] = lo | (hi << 4);
    }
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a.v, b.v, acc, fmt, fmt, 0, scale_a,
                                                         0, scale_b);
  float* out = C + (size_t)wave * 256;
  for (int r = 0; r < 4; r++) {
    int row = (lane >> 4) * 4 + r;
    out[row * 16 + m] = acc[r];
  }
}

// A: [16,128] uint8, B: [128,16] uint8 — raw e4m3 bytes (fmt=0) or fp4 e2m1
// codes 0..15 one-per-byte (fmt=4). scale_a/scale_b: one e8m0 byte each
// (127 = 1.0; 255 is NaN and refused). Returns [waves, 16, 16] fp32 tiles.
torch::Tensor mfma_check_mx(torch::Tensor A, torch::Tensor B, long blocks, long fmt,
                            long scale_a, long scale_b) {
  TORCH_CHECK(A.is_cuda() && B.is_cuda(), "A/B must be on GPU");
  TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8);
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({16, 128}) &&
              B.sizes() == torch::IntArrayRef({128, 16}));
  TORCH_CHECK(fmt == 0 || fmt == 4, "fmt must be 0 (fp8 e4m3) or 4 (fp4 e2m1)");
  TORCH_CHECK(scale_a >= 0 && scale_a <= 254 && scale_b >= 0 && scale_b <= 254,
              "scale_a/scale_b must be e8m0 bytes in 0..254");
  A = A.contiguous();
  B = B.contiguous();
  int threads = 256;
  auto C = tile_output(blocks * (threads / 64), A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  auto kernel = fmt == 0 ? mfma_check_mx_kernel<0> : mfma_check_mx_kernel<4>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, stream, A.data_ptr<unsigned char>(),
                     B.data_ptr<unsigned char>(), C.data_ptr<float>(),
                     (int)(scale_a * 0x01010101L), (int)(scale_b * 0x01010101L));
  HIP_CHECK(hipGetLastError());
  return C;
}

// ---------------------------------------------------------------------------
// LDS integrity: each workgroup fills a 64 KB LDS slab with address-derived
// patterns, barriers, and read-verifies from different lanes (catches
// per-CU LDS faults; HBM and matrix pipes are covered by the other checks).
// ---------------------------------------------------------------------------
__global__ void lds_check_kernel(unsigned long long* __restrict__ errors,
                                 unsigned long long seed) {
  __shared__ unsigned lds[16384];  // 64 KB
  int t = threadIdx.x;
  for (int i = t; i < 16384; i += blockDim.x) {
    lds[i] = (unsigned)(seed ^ (blockIdx.x * 16384u + i) * 2654435761u);
  }
  __syncthreads();
  // verify with a shifted lane mapping so each value is read by a different
  // thread than wrote it (exercises cross-lane LDS paths)
  unsigned long long local = 0;
  for (int i = t; i < 16384; i += blockDim.x) {
    int j = (i + 4097) & 16383;
    unsigned want = (unsigned)(seed ^ (blockIdx.x * 16384u + j) * 2654435761u);
    if (lds[j] != want) local++;
  }
  if (local) atomicAdd(errors, local);
}

// Run the LDS slab check across a grid >> 256 CUs; returns error count.
long lds_check(long blocks, long seed) {
  TORCH_CHECK(blocks > 0);
  DeviceAllocs counter;
  unsigned long long* errs_d =
      static_cast<unsigned long long*>(counter.alloc_zeroed(sizeof(unsigned long long)));
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(lds_check_kernel, dim3(blocks), dim3(256), 0, stream, errs_d,
                     (unsigned long long)seed);
  HIP_CHECK(hipGetLastError());
  // The torch stream is non-blocking: a legacy-stream hipMemcpy would not
  // order against the kernel, racing the error-counter read (a faulty LDS
  // could read back as 0 errors). Synchronize the launch stream first.
  HIP_CHECK(hipStreamSynchronize(stream));
  unsigned long long errs = 0;
  HIP_CHECK(hipMemcpy(&errs, errs_d, sizeof(errs), hipMemcpyDeviceToHost));
  counter.free_all();
  return (long)errs;
}

// ---------------------------------------------------------------------------
// CU coverage: record each wave's hardware placement so the host can verify
// that a health-check grid actually touched every CU on every XCD (a hung or
// fused-off CU shows up as missing coverage): one hw_word() per wave.
// ---------------------------------------------------------------------------
__global__ void cu_coverage_kernel(unsigned* __restrict__ out) {
  const unsigned place = hw_word();
  int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) out[wave] = place;
}

// Returns an int32 tensor of per-wave placement words (hw_word); the host
// derives the set of distinct (xcc, se, sh, cu) tuples.
torch::Tensor cu_coverage(long blocks) {
  TORCH_CHECK(blocks > 0);
  int threads = 256;
  long waves = blocks * (threads / 64);
  auto out = torch::zeros({waves}, torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA));
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(cu_coverage_kernel, dim3(blocks), dim3(threads), 0, stream,
                     reinterpret_cast<unsigned*>(out.data_ptr<int>()));
  HIP_CHECK(hipGetLastError());
  return out;
}

// ---------------------------------------------------------------------------
// MFMA burn-in: a bounded, timed, exactly verifiable run of sustained MFMA
// issue on every CU. The single-tile checks above issue one instruction per
// wave; a matrix pipe that corrupts data only under sustained issue, or a
// GPU that cannot hold its clock, passes them. Here each wave keeps NACC=4
// independent accumulators (A tile i of A[4*16,K] against a shared B[K,16]),
// loads every operand and the expected result into registers once, and then
// for each round zeroes the accumulators, issues `chain` dependent MFMAs per
// accumulator, and compares all four bitwise against `expected`. The hot
// loop has no memory traffic.
//
// Exactness by construction: operands are integers in {-2..2} (exact in
// bf16, e4m3 and e2m1), so every partial sum is an integer of magnitude
// <= 4*K*chain, exact in fp32 while 4*K*chain <= 2^24, and the expected tile
// is chain * (A_i @ B) whatever order the hardware accumulates in.
//
// Lane 0 of each wave writes one int4 record:
//   { placement word (hw_word),
//     mismatched elements over all rounds,
//     first bad round (-1 if none),
//     xor of all accumulator bits over all lanes and rounds }
// so the host can join a wrong result to the CU that produced it.
//
// inject_wave/inject_round (default -1 = off): in that wave, at that round,
// lane 0 flips the lowest mantissa bit of acc[0][0] before the compare.
// Register arithmetic only; it exists to test detection and attribution on
// healthy hardware.
//
// Fragment layouts are those of the checks above (bf16/fp8: 8 K-elements
// per lane; MX: 32 K-elements per lane, fp4 codes one per byte in memory and
// packed low nibble first in registers).
// ---------------------------------------------------------------------------
enum { BURN_BF16 = 0, BURN_FP8 = 1, BURN_MX8 = 2, BURN_MX4 = 3 };
constexpr int BURN_NACC = 4;

template <int FMT> struct BurnMma;

template <> struct BurnMma<BURN_BF16> {
  static constexpr int K = 32;
  typedef frag8 frag;
  static __device__ __forceinline__ frag load_a(const void* A, int row, int lane) {
    const short* p = static_cast<const short*>(A);
    int kbase = (lane >> 4) * 8;
    frag f;
    for (int j = 0; j < 8; j++) f[j] = p[row * 32 + kbase + j];
    return f;
  }
  static __device__ __forceinline__ frag load_b(const void* B, int lane) {
    const short* p = static_cast<const short*>(B);
    int kbase = (lane >> 4) * 8, n = lane & 15;
    frag f;
    for (int j = 0; j < 8; j++) f[j] = p[(kbase + j) * 16 + n];
    return f;
  }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

template <> struct BurnMma<BURN_FP8> {
  static constexpr int K = 32;
  typedef long frag;
  static __device__ __forceinline__ frag load_a(const void* A, int row, int lane) {
    const unsigned char* p = static_cast<const unsigned char*>(A);
    int kbase = (lane >> 4) * 8;
    long f = 0;
    for (int j = 0; j < 8; j++) f |= (long)p[row * 32 + kbase + j] << (8 * j);
    return f;
  }
  static __device__ __forceinline__ frag load_b(const void* B, int lane) {
    const unsigned char* p = static_cast<const unsigned char*>(B);
    int kbase = (lane >> 4) * 8, n = lane & 15;
    long f = 0;
    for (int j = 0; j < 8; j++) f |= (long)p[(kbase + j) * 16 + n] << (8 * j);
    return f;
  }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
  }
};

template <int MXFMT> struct BurnMmaMx {  // MXFMT: 0 = fp8 e4m3, 4 = fp4 e2m1
  static constexpr int K = 128;
  typedef i32x8 frag;
  // element k of this lane's fragment is p[base + k*kstride]: A walks k along
  // a row (kstride 1), B walks k down a column (kstride 16)
  static __device__ __forceinline__ frag load(const unsigned char* p, int lane, int base,
                                              int kstride) {
    int kbase = (lane >> 4) * 32;
    union { i32x8 v; unsigned char b[32]; } f;
    f.v = (i32x8){0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (MXFMT == 0) {
      for (int j = 0; j < 32; j++) f.b[j] = p[base + (kbase + j) * kstride];
    } else {
      for (int j = 0; j < 32; j += 2) {
        unsigned lo = p[base + (kbase + j) * kstride] & 0xF;
        unsigned hi = p[base + (kbase + j + 1) * kstride] & 0xF;
        f.b[j / 2] = lo | (hi << 4);
      }
    }
    return f.v;
  }
  static __device__ __forceinline__ frag load_a(const void* A, int row, int lane) {
    return load(static_cast<const unsigned char*>(A), lane, row * 128, 1);
  }
  static __device__ __forceinline__ frag load_b(const void* B, int lane) {
    return load(static_cast<const unsigned char*>(B), lane, lane & 15, 16);
  }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, MXFMT, MXFMT, 0, 0x7F7F7F7F,
                                                            0, 0x7F7F7F7F);
  }
};
template <> struct BurnMma<BURN_MX8> : BurnMmaMx<0> {};
template <> struct BurnMma<BURN_MX4> : BurnMmaMx<4> {};

template <int FMT>
__global__ void __launch_bounds__(256)
mfma_burn_kernel(const void* __restrict__ A, const void* __restrict__ B,
                 const float* __restrict__ expected, int4* __restrict__ records, int chain,
                 int rounds, int inject_wave, int inject_round) {
  typedef BurnMma<FMT> M;
  int lane = threadIdx.x & 63;
  int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int m = lane & 15;
  const unsigned place = hw_word();

  typename M::frag a[BURN_NACC];
  for (int i = 0; i < BURN_NACC; i++) a[i] = M::load_a(A, i * 16 + m, lane);
  typename M::frag b = M::load_b(B, lane);
  unsigned want[BURN_NACC][4];
  for (int i = 0; i < BURN_NACC; i++)
    for (int r = 0; r < 4; r++)
      want[i][r] = __float_as_uint(expected[i * 256 + ((lane >> 4) * 4 + r) * 16 + m]);

  bool inject_here = (wave == inject_wave) && (lane == 0);
  int mismatched = 0, first_bad = -1;
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    f32x4 acc[BURN_NACC];
#pragma unroll
    for (int i = 0; i < BURN_NACC; i++) {
      acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // opaque to the optimiser: every round really recomputes its chain
      asm volatile("" : "+v"(acc[i]));
    }
    for (int c = 0; c < chain; c++) {
#pragma unroll
      for (int i = 0; i < BURN_NACC; i++) acc[i] = M::mma(a[i], b, acc[i]);
    }
    if (inject_here && round == inject_round)
      acc[0][0] = __uint_as_float(__float_as_uint(acc[0][0]) ^ 1u);
    int bad = 0;
#pragma unroll
    for (int i = 0; i < BURN_NACC; i++) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        unsigned bits = __float_as_uint(acc[i][r]);
        bad += (bits != want[i][r]);
        checksum ^= bits;
      }
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    mismatched += bad;
    if (bad && first_bad < 0) first_bad = round;
  }
  checksum = wave_xor(checksum);
  if (lane == 0) records[wave] = make_int4((int)place, mismatched, first_bad, (int)checksum);
}

// A: [64,K], B: [K,16], expected: [4,16,16] fp32 (= chain * A_i @ B).
// fmt "bf16": bf16 tensors, K=32. "fp8": uint8 raw e4m3 bytes, K=32.
// "mx8": uint8 raw e4m3 bytes, K=128. "mx4": uint8 e2m1 codes one per byte,
// K=128. One untimed warm-up launch, then one timed launch
// (warm_then_timed_ms).
// Returns (records [waves,4] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> mfma_burn(torch::Tensor A, torch::Tensor B,
                                            torch::Tensor expected, const std::string& fmt,
                                            long blocks, long chain, long rounds,
                                            long inject_wave, long inject_round) {
  int f = fmt == "bf16" ? BURN_BF16 : fmt == "fp8" ? BURN_FP8 : fmt == "mx8" ? BURN_MX8
          : fmt == "mx4" ? BURN_MX4 : -1;
  TORCH_CHECK(f >= 0, "fmt must be one of bf16, fp8, mx8, mx4; got ", fmt);
  const long K = (f == BURN_BF16 || f == BURN_FP8) ? 32 : 128;
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && expected.is_cuda(), "A/B/expected must be on GPU");
  TORCH_CHECK(A.device() == B.device() && A.device() == expected.device(),
              "A/B/expected must be on the same device");
  if (f == BURN_BF16) {
    TORCH_CHECK(A.dtype() == torch::kBFloat16 && B.dtype() == torch::kBFloat16,
                "bf16 burn: A/B must be bfloat16");
  } else {
    TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8,
                "fp8/mx8/mx4 burn: A/B must be uint8 (raw e4m3 bytes or e2m1 codes)");
  }
  TORCH_CHECK(expected.dtype() == torch::kFloat32, "expected must be float32");
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({BURN_NACC * 16, K}) &&
                  B.sizes() == torch::IntArrayRef({K, 16}) &&
                  expected.sizes() == torch::IntArrayRef({BURN_NACC, 16, 16}),
              "shapes must be A [64,K], B [K,16], expected [4,16,16] with K=", K);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  // |operand| <= 2, so every partial sum is an integer <= 4*K*chain: exact
  // in fp32 only up to 2^24
  TORCH_CHECK(4 * K * chain <= (1L << 24), "chain ", chain, " breaks fp32 exactness for K=", K,
              " (need 4*K*chain <= 2^24)");
  // bounded run: at most 2^22 MFMAs per accumulator per wave (~2 s at the
  // default grid on the slowest format)
  TORCH_CHECK(rounds <= (1L << 22) && chain * rounds <= (1L << 22),
              "chain*rounds must be <= 2^22");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds,
              "inject_wave/inject_round out of range");
  A = A.contiguous();
  B = B.contiguous();
  expected = expected.contiguous();
  auto records = zero_records(blocks * 4, 4, A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<4>(f, [&](auto fmt_c) {
      hipLaunchKernelGGL((mfma_burn_kernel<decltype(fmt_c)::value>), dim3(blocks), dim3(256), 0,
                         stream, A.data_ptr(), B.data_ptr(), expected.data_ptr<float>(),
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (int)chain, (int)rounds,
                         (int)inject_wave, (int)inject_round);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// MX scale probe: what every real MXFP8/MXFP6/MXFP4 GEMM uses of
// v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4 and the checks above leave
// out: a per-lane E8M0 scale operand, the four-way byte select (op_sel,
// op_sel_hi), different scales in different K blocks, the 6-bit unpackers
// (e2m3, e3m2), the e5m2 decoder, mixed A/B formats (cbsz != blgp) and the
// 32x32x64 shape. mx_scale_tile returns one tile per wave for the host to
// compare bitwise with the float64 product (ops/mx_scale.py); mx_scale_burn
// is the sustained, timed run with the compare in the kernel.
//
// Format codes are the instruction's own: 0 e4m3, 1 e5m2, 2 e2m3, 3 e3m2,
// 4 e2m1. In memory an operand is one code per byte (raw bytes for the 8-bit
// formats, 0..63 and 0..15 for the others).
//
// Layouts (gfx950), with M the tile edge and one lane group = M lanes:
//   16x16x128: lane l has i = l & 15, g = l >> 4 (4 groups);
//              D reg r of 4  -> row 4g + r, col i
//   32x32x64:  lane l has i = l & 31, g = l >> 5 (2 groups);
//              D reg r of 16 -> row 8*(r>>2) + 4g + (r&3), col i
//   K walk:    the lane holds A[i][k(g,j)] and B[k(g,j)][i], j in [0,32).
//              6-bit and 4-bit formats: k = 32g + j, a lane group's K share
//              is exactly one 32-element MX block. 8-bit formats (measured on
//              an MI355X, BENCHMARKS.md "MX scale probe"): the instruction
//              takes VGPRs 0-3 of all groups as the first half of K and VGPRs
//              4-7 as the second, k = (j>>4) * 16G + 16g + (j&15) with G the
//              number of groups, so a lane holds 16 elements of each of two
//              blocks and the scales it applies come from two other lanes.
//              Without per-block scales the walk cannot be observed (A and B
//              permute alike), which is why mfma_check_mx passes with 32g + j.
//   registers: element j of the lane's 32 is byte j of 8 VGPRs (8-bit
//              formats), bits [6j, 6j+6) of a 192-bit little-endian stream
//              in 6 VGPRs (6-bit), bits [4j, 4j+4) of 4 VGPRs (4-bit); the
//              upper registers of the i32x8 operand are zero.
//   scales:    byte `sel` (the instruction's op_sel | op_sel_hi << 1) of the
//              lane's scale VGPR is the E8M0 scale (2^(s-127)) of A's row i,
//              block g; for the B operand of B's column i, block g. The host
//              passes the four bytes a lane holds: scale_a [M, K/32, 4],
//              scale_b [K/32, M, 4].
//
// Fragments are packed in registers straight from global byte loads, with no
// LDS staging: each code is read by exactly one lane, once per launch, so
// there is nothing for LDS to share, and the burn's hot loop touches no
// memory at all. B's loads walk a column (stride M), which neighbouring lanes
// coalesce. Each format of a mixed pair walks K its own way; the instruction
// pairs elements by k.
//
// op_sel is an immediate, so the runtime (sel_a, sel_b) of the tile kernel is
// a wave-uniform switch over the 16 combinations, and the burn's chain is
// unrolled by four with step c issuing op_sel = c & 3 on both sides.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int mx_bits(int fmt) { return fmt <= 1 ? 8 : fmt <= 3 ? 6 : 4; }

template <int SHAPE> struct MxShape;

template <> struct MxShape<0> {  // 16x16x128
  static constexpr int M = 16, LOG_M = 4, K = 128, G = 4, NREG = 4;
  typedef f32x4 acc;
  static __device__ __forceinline__ int row(int r, int g) { return 4 * g + r; }
  template <int FA, int FB, int SEL_A, int SEL_B>
  static __device__ __forceinline__ acc mma(i32x8 a, i32x8 b, acc c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, SEL_A, sa, SEL_B, sb);
  }
};

template <> struct MxShape<1> {  // 32x32x64
  static constexpr int M = 32, LOG_M = 5, K = 64, G = 2, NREG = 16;
  typedef f32x16 acc;
  static __device__ __forceinline__ int row(int r, int g) {
    return 8 * (r >> 2) + 4 * g + (r & 3);
  }
  template <int FA, int FB, int SEL_A, int SEL_B>
  static __device__ __forceinline__ acc mma(i32x8 a, i32x8 b, acc c, int sa, int sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FA, FB, SEL_A, sa, SEL_B, sb);
  }
};

// the lane's 32 codes, packed BITS apiece into the operand: element j is
// p[mx_k<BITS, G>(g, j) * stride]
template <int BITS, int G>
__device__ __forceinline__ constexpr int mx_k(int g, int j) {
  return BITS == 8 ? (j >> 4) * 16 * G + 16 * g + (j & 15) : 32 * g + j;
}

template <int BITS, int G>
__device__ __forceinline__ i32x8 mx_pack(const unsigned char* __restrict__ p, int g, int stride) {
  unsigned w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 32; j++) {
    const unsigned code = p[mx_k<BITS, G>(g, j) * stride] & ((1u << BITS) - 1);
    const int bit = j * BITS, word = bit >> 5, at = bit & 31;
    w[word] |= code << at;
    if (at + BITS > 32) w[word + 1] |= code >> (32 - at);  // a 6-bit code across two VGPRs
  }
  return (i32x8){(int)w[0], (int)w[1], (int)w[2], (int)w[3],
                 (int)w[4], (int)w[5], (int)w[6], (int)w[7]};
}

// one MFMA with the runtime byte selects sel = sel_a * 4 + sel_b (wave-uniform)
template <int SHAPE, int FA, int FB>
__device__ __forceinline__ typename MxShape<SHAPE>::acc
mx_mma_sel(i32x8 a, i32x8 b, typename MxShape<SHAPE>::acc c, int sa, int sb, int sel) {
  typedef MxShape<SHAPE> S;
  switch (sel) {
#define MX_SEL_CASE(n) \
  case n: return S::template mma<FA, FB, ((n) >> 2), ((n) & 3)>(a, b, c, sa, sb);
    MX_SEL_CASE(0) MX_SEL_CASE(1) MX_SEL_CASE(2) MX_SEL_CASE(3)
    MX_SEL_CASE(4) MX_SEL_CASE(5) MX_SEL_CASE(6) MX_SEL_CASE(7)
    MX_SEL_CASE(8) MX_SEL_CASE(9) MX_SEL_CASE(10) MX_SEL_CASE(11)
    MX_SEL_CASE(12) MX_SEL_CASE(13) MX_SEL_CASE(14) MX_SEL_CASE(15)
#undef MX_SEL_CASE
  }
  return c;
}

template <int SHAPE, int FA, int FB>
__global__ void __launch_bounds__(256)
mx_scale_tile_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
                     const int* __restrict__ scale_a, const int* __restrict__ scale_b,
                     float* __restrict__ C, int sel) {
  typedef MxShape<SHAPE> S;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int i = lane & (S::M - 1), g = lane >> S::LOG_M;
  const i32x8 a = mx_pack<mx_bits(FA), S::G>(A + i * S::K, g, 1);
  const i32x8 b = mx_pack<mx_bits(FB), S::G>(B + i, g, S::M);
  const int sa = scale_a[i * S::G + g];
  const int sb = scale_b[g * S::M + i];
  typename S::acc acc;
#pragma unroll
  for (int r = 0; r < S::NREG; r++) acc[r] = 0.f;
  acc = mx_mma_sel<SHAPE, FA, FB>(a, b, acc, sa, sb, sel);
  float* out = C + (size_t)wave * (S::M * S::M);
#pragma unroll
  for (int r = 0; r < S::NREG; r++) out[S::row(r, g) * S::M + i] = acc[r];
}

// the (fmt_a, fmt_b) pairs the kernels are instantiated for, in both shapes
constexpr int MX_PAIRS = 9;
constexpr int MX_PAIR_FMT[MX_PAIRS][2] = {{0, 0}, {1, 1}, {2, 2}, {3, 3}, {4, 4},
                                          {0, 4}, {4, 0}, {2, 1}, {3, 4}};

// what both entry points require of the operands: uint8 on one device, the
// shapes of `rows` stacked A tiles, codes inside each format's width, no NaN
// scale byte, scale tables a lane can read as one dword
static void mx_check_operands(const torch::Tensor& A, const torch::Tensor& B,
                              const torch::Tensor& scale_a, const torch::Tensor& scale_b,
                              long fmt_a, long fmt_b, long shape, long tiles) {
  TORCH_CHECK(shape == 0 || shape == 1, "shape must be 0 (16x16x128) or 1 (32x32x64)");
  TORCH_CHECK(fmt_a >= 0 && fmt_a <= 4 && fmt_b >= 0 && fmt_b <= 4,
              "format codes are 0 e4m3, 1 e5m2, 2 e2m3, 3 e3m2, 4 e2m1");
  const long M = shape == 0 ? 16 : 32, K = shape == 0 ? 128 : 64;
  for (const torch::Tensor* t : {&A, &B, &scale_a, &scale_b}) {
    TORCH_CHECK(t->is_cuda() && t->device() == A.device(),
                "A, B and the scales must be on one GPU");
    TORCH_CHECK(t->dtype() == torch::kUInt8, "A, B and the scales must be uint8");
  }
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({tiles * M, K}) &&
                  B.sizes() == torch::IntArrayRef({K, M}) &&
                  scale_a.sizes() == torch::IntArrayRef({tiles * M, K / 32, 4}) &&
                  scale_b.sizes() == torch::IntArrayRef({K / 32, M, 4}),
              "shapes must be A [", tiles * M, ",", K, "], B [", K, ",", M, "], scale_a [",
              tiles * M, ",", K / 32, ",4], scale_b [", K / 32, ",", M, ",4]");
  TORCH_CHECK(A.max().item<int>() < (1 << mx_bits((int)fmt_a)) &&
                  B.max().item<int>() < (1 << mx_bits((int)fmt_b)),
              "an operand holds a code outside its format's width");
  TORCH_CHECK(scale_a.max().item<int>() < 255 && scale_b.max().item<int>() < 255,
              "scale byte 255 is the E8M0 NaN");
}

static const int* mx_scale_words(const torch::Tensor& scale) {
  auto p = reinterpret_cast<uintptr_t>(scale.data_ptr());
  TORCH_CHECK(p % 4 == 0, "a scale table must be 4-byte aligned");
  return reinterpret_cast<const int*>(p);
}

// A: [M,K], B: [K,M], scale_a: [M,K/32,4], scale_b: [K/32,M,4], all uint8.
// shape 0: M=16, K=128; shape 1: M=32, K=64. Returns [waves, M, M] fp32 tiles.
torch::Tensor mx_scale_tile(torch::Tensor A, torch::Tensor B, torch::Tensor scale_a,
                            torch::Tensor scale_b, long fmt_a, long fmt_b, long shape,
                            long sel_a, long sel_b, long blocks) {
  mx_check_operands(A, B, scale_a, scale_b, fmt_a, fmt_b, shape, 1);
  TORCH_CHECK(sel_a >= 0 && sel_a <= 3 && sel_b >= 0 && sel_b <= 3,
              "sel_a/sel_b select one of the four scale bytes: 0..3");
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  int pair = -1;
  for (int p = 0; p < MX_PAIRS; p++)
    if (MX_PAIR_FMT[p][0] == fmt_a && MX_PAIR_FMT[p][1] == fmt_b) pair = p;
  TORCH_CHECK(pair >= 0, "no kernel for the format pair (", fmt_a, ", ", fmt_b, ")");
  A = A.contiguous();
  B = B.contiguous();
  scale_a = scale_a.contiguous();
  scale_b = scale_b.contiguous();
  const long M = shape == 0 ? 16 : 32;
  auto C = torch::empty({blocks * 4, M, M},
                        torch::TensorOptions().dtype(torch::kFloat32).device(A.device()));
  const int* sa = mx_scale_words(scale_a);
  const int* sb = mx_scale_words(scale_b);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  dispatch_int<2 * MX_PAIRS>((int)shape * MX_PAIRS + pair, [&](auto which) {
    constexpr int W = decltype(which)::value;
    constexpr int SHAPE = W / MX_PAIRS, FA = MX_PAIR_FMT[W % MX_PAIRS][0],
                  FB = MX_PAIR_FMT[W % MX_PAIRS][1];
    hipLaunchKernelGGL((mx_scale_tile_kernel<SHAPE, FA, FB>), dim3(blocks), dim3(256), 0, stream,
                       A.data_ptr<unsigned char>(), B.data_ptr<unsigned char>(), sa, sb,
                       C.data_ptr<float>(), (int)(sel_a * 4 + sel_b));
  });
  HIP_CHECK(hipGetLastError());
  return C;
}

// ---------------------------------------------------------------------------
// MX scale burn: the protocol of mfma_burn (operands, scales and expected
// bits in registers once, no memory traffic in the hot loop, one int4 record
// per wave: {placement word, mismatched elements, first bad round, xor
// checksum}; inject flips the lowest mantissa bit of acc[0][0] in registers)
// with two differences: every lane carries its own four scale bytes, and
// chain step c issues with op_sel = c & 3 on both sides, so sustained issue
// rotates through the byte mux. The chain is unrolled by four (chain % 4 == 0).
//
// Exactness by construction: operands are integers in {-2..2}, scale bytes
// lie in 127 + [-2, 2] per side, so every term is an integer of magnitude
// <= 4 times 2^d, d in [-4, 4]: in units of 2^-4 a partial sum stays below
// 4 * K * chain * 2^8, exact in fp32 while that is <= 2^24. The expected
// tile is (chain / 4) * sum over sel of tile_sel.
//
// Four independent accumulators per wave in both shapes; they live in AGPRs.
// gfx950 build, 256 threads per workgroup, no scratch in any instantiation:
//   16x16x128: 99 VGPRs (e4m3), 90 (e2m3), 84 (e2m1) + 16 AGPRs, 4 waves/SIMD
//   32x32x64:  195 VGPRs (e4m3), 185 (e2m3), 175 (e2m1) + 64 AGPRs, 1 wave per
//              SIMD for e4m3 and 2 for the others, of the 512 registers a
//              lane has; the four accumulators cover the MFMA's latency
// ---------------------------------------------------------------------------
constexpr int MXB_NACC = 4;
constexpr int MXB_FORMATS = 3;
constexpr int MXB_FMT[MXB_FORMATS] = {0, 2, 4};

template <int SHAPE, int FMT>
__global__ void __launch_bounds__(256)
mx_scale_burn_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
                     const int* __restrict__ scale_a, const int* __restrict__ scale_b,
                     const float* __restrict__ expected, int4* __restrict__ records, int chain,
                     int rounds, int inject_wave, int inject_round) {
  typedef MxShape<SHAPE> S;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int i = lane & (S::M - 1), g = lane >> S::LOG_M;
  const unsigned place = hw_word();

  i32x8 a[MXB_NACC];
  int sa[MXB_NACC];
  unsigned want[MXB_NACC][S::NREG];
#pragma unroll
  for (int n = 0; n < MXB_NACC; n++) {
    a[n] = mx_pack<mx_bits(FMT), S::G>(A + (n * S::M + i) * S::K, g, 1);
    sa[n] = scale_a[(n * S::M + i) * S::G + g];
#pragma unroll
    for (int r = 0; r < S::NREG; r++)
      want[n][r] = __float_as_uint(expected[(n * S::M + S::row(r, g)) * S::M + i]);
  }
  const i32x8 b = mx_pack<mx_bits(FMT), S::G>(B + i, g, S::M);
  const int sb = scale_b[g * S::M + i];

  const bool inject_here = (wave == inject_wave) && (lane == 0);
  int mismatched = 0, first_bad = -1;
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    typename S::acc acc[MXB_NACC];
#pragma unroll
    for (int n = 0; n < MXB_NACC; n++) {
#pragma unroll
      for (int r = 0; r < S::NREG; r++) acc[n][r] = 0.f;
      // opaque to the optimiser: every round really recomputes its chain
      asm volatile("" : "+v"(acc[n]));
    }
    for (int c = 0; c < chain; c += 4) {
#pragma unroll
      for (int n = 0; n < MXB_NACC; n++)
        acc[n] = S::template mma<FMT, FMT, 0, 0>(a[n], b, acc[n], sa[n], sb);
#pragma unroll
      for (int n = 0; n < MXB_NACC; n++)
        acc[n] = S::template mma<FMT, FMT, 1, 1>(a[n], b, acc[n], sa[n], sb);
#pragma unroll
      for (int n = 0; n < MXB_NACC; n++)
        acc[n] = S::template mma<FMT, FMT, 2, 2>(a[n], b, acc[n], sa[n], sb);
#pragma unroll
      for (int n = 0; n < MXB_NACC; n++)
        acc[n] = S::template mma<FMT, FMT, 3, 3>(a[n], b, acc[n], sa[n], sb);
    }
    if (inject_here && round == inject_round)
      acc[0][0] = __uint_as_float(__float_as_uint(acc[0][0]) ^ 1u);
    int bad = 0;
#pragma unroll
    for (int n = 0; n < MXB_NACC; n++) {
#pragma unroll
      for (int r = 0; r < S::NREG; r++) {
        const unsigned bits = __float_as_uint(acc[n][r]);
        bad += (bits != want[n][r]);
        checksum ^= bits;
      }
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    mismatched += bad;
    if (bad && first_bad < 0) first_bad = round;
  }
  checksum = wave_xor(checksum);
  if (lane == 0) records[wave] = make_int4((int)place, mismatched, first_bad, (int)checksum);
}

// A: [4M,K], B: [K,M], scale_a: [4M,K/32,4], scale_b: [K/32,M,4] uint8, scale
// bytes in 125..129; expected: [4,M,M] fp32 (= chain/4 * sum over sel of the
// scaled A_n @ B). fmt 0 e4m3, 2 e2m3 or 4 e2m1 on both sides. One untimed
// warm-up launch, then one timed launch (warm_then_timed_ms).
// Returns (records [waves,4] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> mx_scale_burn(torch::Tensor A, torch::Tensor B,
                                                torch::Tensor scale_a, torch::Tensor scale_b,
                                                torch::Tensor expected, long fmt, long shape,
                                                long blocks, long chain, long rounds,
                                                long inject_wave, long inject_round) {
  mx_check_operands(A, B, scale_a, scale_b, fmt, fmt, shape, MXB_NACC);
  int f = -1;
  for (int k = 0; k < MXB_FORMATS; k++)
    if (MXB_FMT[k] == fmt) f = k;
  TORCH_CHECK(f >= 0, "the burn runs formats 0 (e4m3), 2 (e2m3) and 4 (e2m1); got ", fmt);
  const long M = shape == 0 ? 16 : 32, K = shape == 0 ? 128 : 64;
  TORCH_CHECK(expected.is_cuda() && expected.device() == A.device() &&
                  expected.dtype() == torch::kFloat32 &&
                  expected.sizes() == torch::IntArrayRef({MXB_NACC, M, M}),
              "expected must be float32 [4,", M, ",", M, "] on the operands' GPU");
  TORCH_CHECK(scale_a.min().item<int>() >= 125 && scale_a.max().item<int>() <= 129 &&
                  scale_b.min().item<int>() >= 125 && scale_b.max().item<int>() <= 129,
              "burn scale bytes must lie in 125..129");
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(chain >= 4 && chain % 4 == 0 && rounds >= 1,
              "chain must be a positive multiple of 4 and rounds >= 1");
  // |operand| <= 2 and scales 2^[-2,2] per side: a partial sum is an integer
  // <= 4*K*chain*2^8 in units of 2^-4, exact in fp32 only up to 2^24
  TORCH_CHECK(4 * K * chain * 256 <= (1L << 24), "chain ", chain,
              " breaks fp32 exactness for K=", K, " (need 4*K*chain*2^8 <= 2^24)");
  TORCH_CHECK(rounds <= (1L << 22) && chain * rounds <= (1L << 22),
              "chain*rounds must be <= 2^22");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds,
              "inject_wave/inject_round out of range");
  A = A.contiguous();
  B = B.contiguous();
  scale_a = scale_a.contiguous();
  scale_b = scale_b.contiguous();
  expected = expected.contiguous();
  const int* sa = mx_scale_words(scale_a);
  const int* sb = mx_scale_words(scale_b);
  auto records = zero_records(blocks * 4, 4, A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<2 * MXB_FORMATS>((int)shape * MXB_FORMATS + f, [&](auto which) {
      constexpr int W = decltype(which)::value;
      hipLaunchKernelGGL((mx_scale_burn_kernel<W / MXB_FORMATS, MXB_FMT[W % MXB_FORMATS]>),
                         dim3(blocks), dim3(256), 0, stream, A.data_ptr<unsigned char>(),
                         B.data_ptr<unsigned char>(), sa, sb, expected.data_ptr<float>(),
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (int)chain, (int)rounds,
                         (int)inject_wave, (int)inject_round);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// Matrix-path probe: the matrix instructions tenant jobs run and no probe
// above issues. Dense: f64 16x16x4 (every DGEMM), f32 16x16x4 and 32x32x2,
// f16 16x16x32 and 32x32x16, bf16 and e4m3 in the 32x32x16 shape, i8 to i32
// in 16x16x64 and 32x32x32, e5m2 and the two mixed e4m3/e5m2 forms of the
// unscaled 8-bit MFMA. Sparse: the 2:4 structured v_smfmac_* in f16 (16x16x64,
// 32x32x32), bf16 (16x16x64) and i8 (16x16x128), with their index operand and
// its part select. matrix_tile returns one tile per wave for the host to
// compare bitwise with the float64 / int64 product (ops/matrix_paths.py);
// matrix_burn is the sustained, timed run with the compare in the kernel.
//
// One trait per path (MatPath<PATH>, below) gives the element and fragment
// types, load_a, load_b, mma and the output map; both kernels are written
// once against it.
//
// Layouts (gfx950). M is the tile edge, a lane group is M lanes, G = 64/M
// groups; lane l has i = l % M, g = l / M:
//   A:   the lane holds row i of A, its KA = K/G elements A[i][KA*g + j]
//        (sparse: of the compressed row, KA = K/2/G)
//   B:   the lane holds column i of B, its KB = K/G elements B[kb(g, j)][i];
//        dense: kb = KB*g + j. Sparse (measured on an MI355X with one-hot
//        operands, BENCHMARKS.md "Matrix-path probe"): the first four VGPRs
//        of all groups are the first half of K and the last four the second,
//        kb = (j / H) * H*G + H*g + j % H with H = KB/2, the walk the 8-bit MX
//        operands showed; A's compressed row stays consecutive.
//   D:   16x16: reg r of 4  -> row 4g + r, col i
//        32x32: reg r of 16 -> row 8*(r>>2) + 4g + (r&3), col i
//        f64 16x16x4 (measured, BENCHMARKS.md "Matrix-path probe"): element
//        r of 4, a register pair, -> row 4r + g, col i: a lane's four rows
//        are 4 apart, not consecutive as in the 32-bit 16x16 shapes
//   K:   a dense product does not change when A and B walk K by the same
//        map, so which k the hardware calls register element j of group g
//        cannot be seen from outside; the loaders above are "consecutive" and
//        the one-hot cases (matrix_k_slot_case) prove that load_a and load_b
//        name the same slot, element for element, in every path.
//   2:4: a sparse A row is K/2 values plus, per value, its position 0..3 in
//        its group of four along K (two values per group, positions strictly
//        increasing). Register element j of A pairs with register element
//        4*(j>>1) + position of B in the same lane group: the selection is
//        made on the B registers of the group, so here the walk can be seen.
//        The positions are packed two bits apiece, element j at bits
//        [2j, 2j+2) of the part of the index VGPR that ABID selects: 16 bits
//        per part for the 16-bit paths (KA = 8; ABID 0 reads [15:0], 1 reads
//        [31:16]), all 32 bits for i8 (KA = 16). The parts ABID does not select
//        are filled with another valid pattern (pair (0,1) becomes (2,3), every
//        other pair (0,1)), so a wrong select gives a wrong tile.
//
// Operands go from global memory straight into registers, once per launch;
// the burn's hot loop touches no memory.
//
// Burn protocol: that of mfma_burn (four independent accumulator tiles per
// wave, `chain` dependent MFMAs per accumulator per round, accumulators reset
// through an opaque asm each round, every element compared bitwise, one int4
// record per wave {placement word, mismatched elements, first bad round, xor
// checksum}; inject flips the lowest bit of acc[0][0] of lane 0 in registers).
// Operands are integers of magnitude <= 2, so a partial sum is an integer of
// magnitude <= 4*K*chain: exact while that stays within 2^24 (f32
// accumulators), 2^53 (f64) or 2^31 (i32).
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) double f64x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) _Float16 f16x16;
typedef __attribute__((ext_vector_type(16))) short frag16;

enum {
  MAT_F64_16, MAT_F32_16, MAT_F32_32, MAT_F16_16, MAT_F16_32, MAT_BF16_32, MAT_I8_16, MAT_I8_32,
  MAT_FP8_32, MAT_BF8_16, MAT_FP8BF8_16, MAT_BF8FP8_16,
  MAT_SP_F16_16, MAT_SP_F16_32, MAT_SP_BF16_16, MAT_SP_I8_16, MAT_PATHS
};
constexpr int MAT_NACC = 4;

// E: element as it lies in memory and in the fragment; FA, FB: the operand
// registers; ACC, OUT: the accumulator vector and its element
template <typename E, typename FA, typename FB, typename ACC, typename OUT, int M_, int K_,
          bool SPARSE_>
struct MatShape {
  static constexpr int M = M_, K = K_, G = 64 / M_, NREG = M_ * M_ / 64;
  static constexpr bool SPARSE = SPARSE_;
  static constexpr int KA = (SPARSE_ ? K_ / 2 : K_) / G, KB = K_ / G;
  typedef FA frag_a;
  typedef FB frag_b;
  typedef ACC acc;
  typedef OUT out;
  static_assert(sizeof(FA) == KA * sizeof(E) && sizeof(FB) == KB * sizeof(E),
                "a fragment is the lane's share of K");
  static __device__ __forceinline__ int row(int r, int g) {
    if (sizeof(OUT) == 8) return 4 * r + g;
    return M == 16 ? 4 * g + r : 8 * (r >> 2) + 4 * g + (r & 3);
  }
  static __device__ __forceinline__ FA load_a(const void* A, int row, int g) {
    const E* p = static_cast<const E*>(A) + row * (KA * G) + KA * g;
    union { FA v; E e[KA]; } f;
#pragma unroll
    for (int j = 0; j < KA; j++) f.e[j] = p[j];
    return f.v;
  }
  // the row of B that register element j of lane group g holds
  static __device__ __forceinline__ constexpr int kb(int g, int j) {
    if constexpr (SPARSE_) {
      constexpr int HALF = KB / 2;
      return (j / HALF) * (HALF * G) + HALF * g + j % HALF;
    } else {
      return KB * g + j;
    }
  }
  static __device__ __forceinline__ FB load_b(const void* B, int col, int g) {
    const E* p = static_cast<const E*>(B) + col;
    union { FB v; E e[KB]; } f;
#pragma unroll
    for (int j = 0; j < KB; j++) f.e[j] = p[kb(g, j) * M];
    return f.v;
  }
};

template <int PATH> struct MatPath;
#define MAT_DENSE(PATH, E, F, ACC, OUT, M, K, INSTR)                                         \
  template <> struct MatPath<PATH> : MatShape<E, F, F, ACC, OUT, M, K, false> {             \
    template <int ABID> static __device__ __forceinline__ ACC mma(F a, F b, ACC c, int) {   \
      return __builtin_amdgcn_mfma_##INSTR(a, b, c, 0, 0, 0);                                \
    }                                                                                        \
  }
#define MAT_SPARSE(PATH, E, FA, FB, ACC, OUT, M, K, INSTR)                                   \
  template <> struct MatPath<PATH> : MatShape<E, FA, FB, ACC, OUT, M, K, true> {            \
    template <int ABID> static __device__ __forceinline__ ACC mma(FA a, FB b, ACC c,        \
                                                                  int index) {              \
      return __builtin_amdgcn_smfmac_##INSTR(a, b, c, index, 0, ABID);                       \
    }                                                                                        \
  }
MAT_DENSE(MAT_F64_16, double, double, f64x4, double, 16, 4, f64_16x16x4f64);
MAT_DENSE(MAT_F32_16, float, float, f32x4, float, 16, 4, f32_16x16x4f32);
MAT_DENSE(MAT_F32_32, float, float, f32x16, float, 32, 2, f32_32x32x2f32);
MAT_DENSE(MAT_F16_16, _Float16, f16x8, f32x4, float, 16, 32, f32_16x16x32_f16);
MAT_DENSE(MAT_F16_32, _Float16, f16x8, f32x16, float, 32, 16, f32_32x32x16_f16);
MAT_DENSE(MAT_BF16_32, short, frag8, f32x16, float, 32, 16, f32_32x32x16_bf16);
MAT_DENSE(MAT_I8_16, signed char, i32x4, i32x4, int, 16, 64, i32_16x16x64_i8);
MAT_DENSE(MAT_I8_32, signed char, i32x4, i32x16, int, 32, 32, i32_32x32x32_i8);
MAT_DENSE(MAT_FP8_32, unsigned char, long, f32x16, float, 32, 16, f32_32x32x16_fp8_fp8);
MAT_DENSE(MAT_BF8_16, unsigned char, long, f32x4, float, 16, 32, f32_16x16x32_bf8_bf8);
MAT_DENSE(MAT_FP8BF8_16, unsigned char, long, f32x4, float, 16, 32, f32_16x16x32_fp8_bf8);
MAT_DENSE(MAT_BF8FP8_16, unsigned char, long, f32x4, float, 16, 32, f32_16x16x32_bf8_fp8);
MAT_SPARSE(MAT_SP_F16_16, _Float16, f16x8, f16x16, f32x4, float, 16, 64, f32_16x16x64_f16);
MAT_SPARSE(MAT_SP_F16_32, _Float16, f16x8, f16x16, f32x16, float, 32, 32, f32_32x32x32_f16);
MAT_SPARSE(MAT_SP_BF16_16, short, frag8, frag16, f32x4, float, 16, 64, f32_16x16x64_bf16);
MAT_SPARSE(MAT_SP_I8_16, signed char, i32x4, i32x8, i32x4, int, 16, 128, i32_16x16x128_i8);
#undef MAT_DENSE
#undef MAT_SPARSE

// the index VGPR of a sparse path from the lane's KA positions (layout above)
template <int KA>
__device__ __forceinline__ int mat_pack_index(const unsigned char* __restrict__ pos, int abid) {
  unsigned own = 0, other = 0;
#pragma unroll
  for (int j = 0; j < KA; j += 2) {
    const unsigned p0 = pos[j] & 3, p1 = pos[j + 1] & 3;
    own |= (p0 | (p1 << 2)) << (2 * j);
    other |= ((p0 == 0 && p1 == 1) ? 0xEu : 0x4u) << (2 * j);  // (2,3), else (0,1)
  }
  if constexpr (KA == 16) return (int)own;  // all 32 bits are one part
  return abid == 0 ? (int)(own | (other << 16)) : (int)(other | (own << 16));
}

// an accumulator element's bits, their fold into the 32-bit checksum, and the
// element with its lowest bit flipped
__device__ __forceinline__ unsigned long long mat_bits(double v) {
  return (unsigned long long)__double_as_longlong(v);
}
__device__ __forceinline__ unsigned mat_bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned mat_bits(int v) { return (unsigned)v; }
__device__ __forceinline__ unsigned mat_fold(unsigned long long b) {
  return (unsigned)b ^ (unsigned)(b >> 32);
}
__device__ __forceinline__ unsigned mat_fold(unsigned b) { return b; }
__device__ __forceinline__ double mat_flip(double v) {
  return __longlong_as_double(__double_as_longlong(v) ^ 1LL);
}
__device__ __forceinline__ float mat_flip(float v) {
  return __uint_as_float(__float_as_uint(v) ^ 1u);
}
__device__ __forceinline__ int mat_flip(int v) { return v ^ 1; }

template <int PATH, int ABID>
__global__ void __launch_bounds__(256)
matrix_tile_kernel(const void* __restrict__ A, const void* __restrict__ B,
                   const unsigned char* __restrict__ index, void* __restrict__ C) {
  typedef MatPath<PATH> P;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int i = lane % P::M, g = lane / P::M;
  const typename P::frag_a a = P::load_a(A, i, g);
  const typename P::frag_b b = P::load_b(B, i, g);
  int idx = 0;
  if constexpr (P::SPARSE) idx = mat_pack_index<P::KA>(index + i * (P::KA * P::G) + P::KA * g, ABID);
  typename P::acc acc;
#pragma unroll
  for (int r = 0; r < P::NREG; r++) acc[r] = 0;
  acc = P::template mma<ABID>(a, b, acc, idx);
  typename P::out* out = static_cast<typename P::out*>(C) + (size_t)wave * (P::M * P::M);
#pragma unroll
  for (int r = 0; r < P::NREG; r++) out[P::row(r, g) * P::M + i] = acc[r];
}

template <int PATH, int ABID>
__global__ void __launch_bounds__(256)
matrix_burn_kernel(const void* __restrict__ A, const void* __restrict__ B,
                   const unsigned char* __restrict__ index, const void* __restrict__ expected,
                   int4* __restrict__ records, int chain, int rounds, int inject_wave,
                   int inject_round) {
  typedef MatPath<PATH> P;
  typedef decltype(mat_bits(typename P::out())) bits_t;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int i = lane % P::M, g = lane / P::M;
  const unsigned place = hw_word();

  typename P::frag_a a[MAT_NACC];
  int idx[MAT_NACC];
  bits_t want[MAT_NACC][P::NREG];
  const typename P::out* tile = static_cast<const typename P::out*>(expected);
#pragma unroll
  for (int n = 0; n < MAT_NACC; n++) {
    const int row = n * P::M + i;
    a[n] = P::load_a(A, row, g);
    idx[n] = 0;
    if constexpr (P::SPARSE)
      idx[n] = mat_pack_index<P::KA>(index + row * (P::KA * P::G) + P::KA * g, ABID);
#pragma unroll
    for (int r = 0; r < P::NREG; r++)
      want[n][r] = mat_bits(tile[(n * P::M + P::row(r, g)) * P::M + i]);
  }
  const typename P::frag_b b = P::load_b(B, i, g);

  const bool inject_here = (wave == inject_wave) && (lane == 0);
  int mismatched = 0, first_bad = -1;
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    typename P::acc acc[MAT_NACC];
#pragma unroll
    for (int n = 0; n < MAT_NACC; n++) {
#pragma unroll
      for (int r = 0; r < P::NREG; r++) acc[n][r] = 0;
      // opaque to the optimiser: every round really recomputes its chain
      asm volatile("" : "+v"(acc[n]));
    }
    for (int c = 0; c < chain; c++) {
#pragma unroll
      for (int n = 0; n < MAT_NACC; n++) acc[n] = P::template mma<ABID>(a[n], b, acc[n], idx[n]);
    }
    if (inject_here && round == inject_round) acc[0][0] = mat_flip(acc[0][0]);
    int bad = 0;
#pragma unroll
    for (int n = 0; n < MAT_NACC; n++) {
#pragma unroll
      for (int r = 0; r < P::NREG; r++) {
        const bits_t bits = mat_bits(acc[n][r]);
        bad += (bits != want[n][r]);
        checksum ^= mat_fold(bits);
      }
    }
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off);
    mismatched += bad;
    if (bad && first_bad < 0) first_bad = round;
  }
  checksum = wave_xor(checksum);
  if (lane == 0) records[wave] = make_int4((int)place, mismatched, first_bad, (int)checksum);
}

// what the host knows of a path; the order is that of the MAT_* ids
struct MatInfo {
  const char* name;
  long M, K;
  bool sparse;
  c10::ScalarType in, out;
};
static const MatInfo MAT_INFO[MAT_PATHS] = {
    {"f64_16x16x4", 16, 4, false, torch::kFloat64, torch::kFloat64},
    {"f32_16x16x4", 16, 4, false, torch::kFloat32, torch::kFloat32},
    {"f32_32x32x2", 32, 2, false, torch::kFloat32, torch::kFloat32},
    {"f16_16x16x32", 16, 32, false, torch::kFloat16, torch::kFloat32},
    {"f16_32x32x16", 32, 16, false, torch::kFloat16, torch::kFloat32},
    {"bf16_32x32x16", 32, 16, false, torch::kBFloat16, torch::kFloat32},
    {"i8_16x16x64", 16, 64, false, torch::kInt8, torch::kInt32},
    {"i8_32x32x32", 32, 32, false, torch::kInt8, torch::kInt32},
    {"fp8_32x32x16", 32, 16, false, torch::kUInt8, torch::kFloat32},
    {"bf8_16x16x32", 16, 32, false, torch::kUInt8, torch::kFloat32},
    {"fp8bf8_16x16x32", 16, 32, false, torch::kUInt8, torch::kFloat32},
    {"bf8fp8_16x16x32", 16, 32, false, torch::kUInt8, torch::kFloat32},
    {"sp_f16_16x16x64", 16, 64, true, torch::kFloat16, torch::kFloat32},
    {"sp_f16_32x32x32", 32, 32, true, torch::kFloat16, torch::kFloat32},
    {"sp_bf16_16x16x64", 16, 64, true, torch::kBFloat16, torch::kFloat32},
    {"sp_i8_16x16x128", 16, 128, true, torch::kInt8, torch::kInt32},
};
// the paths the burn kernel is instantiated for
constexpr int MAT_BURN_PATHS = 6;
constexpr int MAT_BURN_PATH[MAT_BURN_PATHS] = {MAT_F64_16, MAT_F32_32, MAT_F16_16,
                                               MAT_I8_16,  MAT_BF8_16, MAT_SP_F16_16};

// The path's id after checking what both entry points require: a known path,
// A [tiles*M, K] (sparse: [tiles*M, K/2] values and as many uint8 positions,
// each below 4 and increasing within a pair) and B [K, M] of the path's type
// on one GPU, abid 0 or 1 and only for a sparse path, blocks in range.
static int mat_check_operands(const std::string& path, const torch::Tensor& A,
                              const torch::Tensor& B,
                              const c10::optional<torch::Tensor>& index, long abid, long blocks,
                              long tiles) {
  int id = -1;
  for (int p = 0; p < MAT_PATHS; p++)
    if (path == MAT_INFO[p].name) id = p;
  TORCH_CHECK(id >= 0, "unknown matrix path ", path);
  const MatInfo& info = MAT_INFO[id];
  const long ka = info.sparse ? info.K / 2 : info.K;
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && A.device() == B.device(),
              "A and B must be on one GPU");
  TORCH_CHECK(A.scalar_type() == info.in && B.scalar_type() == info.in, path,
              ": A and B must be ", c10::toString(info.in));
  TORCH_CHECK(A.sizes() == torch::IntArrayRef({tiles * info.M, ka}) &&
                  B.sizes() == torch::IntArrayRef({info.K, info.M}),
              path, ": shapes must be A [", tiles * info.M, ",", ka, "], B [", info.K, ",",
              info.M, "]");
  TORCH_CHECK(index.has_value() == info.sparse, path,
              info.sparse ? ": a sparse path needs `index`" : ": a dense path takes no `index`");
  if (info.sparse) {
    const torch::Tensor& ix = *index;
    TORCH_CHECK(ix.is_cuda() && ix.device() == A.device() && ix.scalar_type() == torch::kUInt8 &&
                    ix.sizes() == A.sizes(),
                path, ": index must be uint8 of A's shape on A's GPU");
    TORCH_CHECK(ix.max().item<int>() < 4 &&
                    ix.slice(1, 0, ka, 2).lt(ix.slice(1, 1, ka, 2)).all().item<bool>(),
                path, ": index holds positions 0..3, increasing within each pair");
  }
  TORCH_CHECK(abid == 0 || (info.sparse && abid == 1), path,
              ": abid must be 0, or 1 on a sparse path");
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  return id;
}

// largest exact `chain` of a path's burn: 4*K*chain within the accumulator's
// integers, and at most the 2^22 MFMAs of a bounded run
static long mat_chain_limit(const MatInfo& info) {
  const long bound = info.out == torch::kFloat64 ? (1L << 53)
                     : info.out == torch::kFloat32 ? (1L << 24) : (1L << 31);
  return std::min(bound / (4 * info.K), 1L << 22);
}

static const unsigned char* mat_index_ptr(const c10::optional<torch::Tensor>& index) {
  return index.has_value() ? index->data_ptr<unsigned char>() : nullptr;
}

// A: [M,K] (sparse [M,K/2] with index [M,K/2] uint8), B: [K,M].
// Returns [waves, M, M] tiles in the accumulator's type.
torch::Tensor matrix_tile(const std::string& path, torch::Tensor A, torch::Tensor B, long blocks,
                          c10::optional<torch::Tensor> index, long abid) {
  const int id = mat_check_operands(path, A, B, index, abid, blocks, 1);
  const MatInfo& info = MAT_INFO[id];
  A = A.contiguous();
  B = B.contiguous();
  if (index.has_value()) index = index->contiguous();
  auto C = torch::empty({blocks * 4, info.M, info.M},
                        torch::TensorOptions().dtype(info.out).device(A.device()));
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  dispatch_int<MAT_PATHS>(id, [&](auto path_c) {
    constexpr int PATH = decltype(path_c)::value;
    dispatch_int<MatPath<PATH>::SPARSE ? 2 : 1>((int)abid, [&](auto abid_c) {
      hipLaunchKernelGGL((matrix_tile_kernel<PATH, decltype(abid_c)::value>), dim3(blocks),
                         dim3(256), 0, stream, A.data_ptr(), B.data_ptr(), mat_index_ptr(index),
                         C.data_ptr());
    });
  });
  HIP_CHECK(hipGetLastError());
  return C;
}

// A: [4M,K] (sparse [4M,K/2] with index), B: [K,M], expected: [4,M,M] in the
// accumulator's type (= chain * A_n @ B), operands integers of magnitude <= 2.
// One untimed warm-up launch, then one timed launch (warm_then_timed_ms).
// Returns (records [waves,4] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> matrix_burn(const std::string& path, torch::Tensor A,
                                              torch::Tensor B, torch::Tensor expected, long blocks,
                                              long chain, long rounds, long inject_wave,
                                              long inject_round,
                                              c10::optional<torch::Tensor> index, long abid) {
  const int id = mat_check_operands(path, A, B, index, abid, blocks, MAT_NACC);
  const MatInfo& info = MAT_INFO[id];
  int which = -1;
  for (int k = 0; k < MAT_BURN_PATHS; k++)
    if (MAT_BURN_PATH[k] == id) which = k;
  TORCH_CHECK(which >= 0, "no burn kernel for the path ", path);
  TORCH_CHECK(expected.is_cuda() && expected.device() == A.device() &&
                  expected.scalar_type() == info.out &&
                  expected.sizes() == torch::IntArrayRef({MAT_NACC, info.M, info.M}),
              path, ": expected must be ", c10::toString(info.out), " [4,", info.M, ",", info.M,
              "] on the operands' GPU");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  TORCH_CHECK(chain <= mat_chain_limit(info), "chain ", chain, " breaks exactness for ", path,
              " (limit ", mat_chain_limit(info), ")");
  TORCH_CHECK(rounds <= (1L << 22) && chain * rounds <= (1L << 22),
              "chain*rounds must be <= 2^22");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds,
              "inject_wave/inject_round out of range");
  A = A.contiguous();
  B = B.contiguous();
  expected = expected.contiguous();
  if (index.has_value()) index = index->contiguous();
  auto records = zero_records(blocks * 4, 4, A.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<MAT_BURN_PATHS>(which, [&](auto which_c) {
      constexpr int PATH = MAT_BURN_PATH[decltype(which_c)::value];
      dispatch_int<MatPath<PATH>::SPARSE ? 2 : 1>((int)abid, [&](auto abid_c) {
        hipLaunchKernelGGL((matrix_burn_kernel<PATH, decltype(abid_c)::value>), dim3(blocks),
                           dim3(256), 0, stream, A.data_ptr(), B.data_ptr(), mat_index_ptr(index),
                           expected.data_ptr(), reinterpret_cast<int4*>(records.data_ptr<int>()),
                           (int)chain, (int)rounds, (int)inject_wave, (int)inject_round);
      });
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// LDS march: a timed write/read-verify of the WHOLE 160 KiB LDS of a CU, in
// both bit polarities and through both the narrow and the wide read path,
// with the location and direction of any mismatch recorded per wave.
// lds_check above touches a 64 KiB slab once with one value per word; this
// kernel declares all 163840 B statically, so at most one workgroup is
// resident per CU and that workgroup owns every byte of the CU's LDS.
//
// Pattern: p(round, i) = fmix32((seed + round*0x9E3779B9) ^ (i*0x85EBCA6B)),
// fmix32 the murmur3 finaliser. The multiply by an odd constant, the xor and
// fmix32 are bijections on 32 bits, so within a pass all 40960 words hold
// distinct values and an address-decoder alias (two indices reaching one
// cell) reads back as a data mismatch.
//
// Each round runs four passes (global pass index = round*4 + phase); word i
// is always written by thread i mod 256 with ds_write_b32:
//   phase 0: write  p, read b32, thread t reads words j = t+65 (mod 256)
//   phase 1: write ~p, read b32, same mapping
//   phase 2: write  p, read b128 (uint4), thread t reads quads q = t (mod 256)
//   phase 3: write ~p, read b128
// 40960 = 160*256, so in the b32 passes every word is read by lane+1 of
// another wave than the one that wrote it. A barrier separates each write
// from its read and each read from the next write. After the four passes
// every bit of every word has been verified holding 0 and holding 1 through
// ds_read_b32 and through ds_read_b128 (checked in the gfx950 disassembly:
// the phase 2/3 loop issues ds_read_b128, the phase 0/1 loop ds_read_b32 and
// the writes ds_write_b32).
//
// No LDS is left for a reduction: each wave reduces with shuffles and lane 0
// writes its own record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched dwords over all passes
//   [2] first bad global pass index (-1 if none)
//   [3] lowest mismatching word index within that pass (-1 if none)
//   [4] dropped mask: OR of (want & ~got), bits that should be 1 and read 0
//   [5] raised mask:  OR of (got & ~want), bits that should be 0 and read 1
//   [6] sum mod 2^32 of every dword this wave read in phases 0 and 2
//   [7] 0 (reserved)
// The host combines the four waves of a block.
//
// inject_* (default -1 = off): in block inject_block, at global pass
// inject_pass, after that pass's write and barrier, thread 0 flips bit
// inject_bit of lds[inject_word]; an extra barrier follows and the read
// proceeds. A plain store into the workgroup's own LDS: it sends a known
// one-bit fault through the real read-and-compare path on healthy hardware.
// ---------------------------------------------------------------------------
constexpr int LDS_MARCH_WORDS = 40960;  // 163840 B: the whole LDS of a CU
constexpr int LDS_MARCH_THREADS = 256;  // four waves, one per SIMD
// accesses per thread and batch; 160 words and 40 quads per thread and pass
constexpr int LDS_MARCH_BATCH = 8;
constexpr int LDS_MARCH_WIDE_BATCH = 4;
static_assert(LDS_MARCH_WORDS % (LDS_MARCH_BATCH * LDS_MARCH_THREADS) == 0 &&
                  (LDS_MARCH_WORDS / 4) % (LDS_MARCH_WIDE_BATCH * LDS_MARCH_THREADS) == 0,
              "batches must tile the LDS exactly");

__device__ __forceinline__ unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// p(round, i) with rs = seed + round*0x9E3779B9
__device__ __forceinline__ unsigned lds_march_pattern(unsigned rs, int i) {
  return fmix32(rs ^ ((unsigned)i * 0x85EBCA6Bu));
}

struct LdsMarchState {
  int mismatched, first_pass, first_word;
  unsigned dropped, raised;
};

// a thread visits its words in ascending order within a pass, so the first
// mismatch it sees in its first bad pass is its lowest
__device__ __forceinline__ void lds_march_compare(LdsMarchState& s, unsigned got, unsigned want,
                                                  int pass, int word) {
  // branch-free, so the unrolled read loops keep their LDS reads in flight
  const unsigned diff = got ^ want;
  const bool bad = diff != 0;
  const bool first = bad && s.first_pass < 0;
  s.mismatched += bad;
  s.dropped |= want & diff;
  s.raised |= got & diff;
  s.first_pass = first ? pass : s.first_pass;
  s.first_word = first ? word : s.first_word;
}

__global__ void __launch_bounds__(LDS_MARCH_THREADS)
lds_march_kernel(int4* __restrict__ records, int rounds, unsigned seed, int inject_block,
                 int inject_word, int inject_pass, int inject_bit) {
  __shared__ __attribute__((aligned(16))) unsigned lds[LDS_MARCH_WORDS];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int wave = blockIdx.x * (LDS_MARCH_THREADS >> 6) + (t >> 6);
  const unsigned place = hw_word();

  const bool inject_block_here = (int)blockIdx.x == inject_block &&
                                 (unsigned)inject_word < (unsigned)LDS_MARCH_WORDS;
  const int tr = (t + 65) & (LDS_MARCH_THREADS - 1);  // b32 read mapping
  LdsMarchState s = {0, -1, -1, 0u, 0u};
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    const unsigned rs = seed + (unsigned)round * 0x9E3779B9u;
    for (int phase = 0; phase < 4; phase++) {
      const int pass = round * 4 + phase;
      const unsigned inv = (phase & 1) ? 0xFFFFFFFFu : 0u;
      const unsigned sum_mask = (phase & 1) ? 0u : 0xFFFFFFFFu;
      // Batches of LDS_MARCH_BATCH accesses per thread: the values of a batch
      // are hashed (or compared) in registers around one run of LDS
      // instructions, so several are in flight per wave. The empty asm
      // between two accesses keeps each one a single ds_write_b32 /
      // ds_read_b32: the compiler otherwise pairs the strided accesses into
      // ds_write2st64_b32 / ds_read2st64_b32.
      for (int base = t; base < LDS_MARCH_WORDS; base += LDS_MARCH_BATCH * LDS_MARCH_THREADS) {
        unsigned val[LDS_MARCH_BATCH];
#pragma unroll
        for (int k = 0; k < LDS_MARCH_BATCH; k++)
          val[k] = lds_march_pattern(rs, base + k * LDS_MARCH_THREADS) ^ inv;
#pragma unroll
        for (int k = 0; k < LDS_MARCH_BATCH; k++) {
          lds[base + k * LDS_MARCH_THREADS] = val[k];
          asm volatile("" ::: "memory");
        }
      }
      __syncthreads();
      if (inject_block_here && pass == inject_pass) {  // block-uniform
        if (t == 0) lds[inject_word] ^= 1u << inject_bit;
        __syncthreads();
      }
      if (phase < 2) {
        for (int base = tr; base < LDS_MARCH_WORDS; base += LDS_MARCH_BATCH * LDS_MARCH_THREADS) {
          unsigned got[LDS_MARCH_BATCH];
#pragma unroll
          for (int k = 0; k < LDS_MARCH_BATCH; k++) {
            got[k] = lds[base + k * LDS_MARCH_THREADS];
            asm volatile("" ::: "memory");
          }
#pragma unroll
          for (int k = 0; k < LDS_MARCH_BATCH; k++) {
            int j = base + k * LDS_MARCH_THREADS;
            checksum += got[k] & sum_mask;
            lds_march_compare(s, got[k], lds_march_pattern(rs, j) ^ inv, pass, j);
          }
        }
      } else {
        const uint4* quads = reinterpret_cast<const uint4*>(lds);
        for (int base = t; base < LDS_MARCH_WORDS / 4;
             base += LDS_MARCH_WIDE_BATCH * LDS_MARCH_THREADS) {
          uint4 got[LDS_MARCH_WIDE_BATCH];
#pragma unroll
          for (int k = 0; k < LDS_MARCH_WIDE_BATCH; k++)
            got[k] = quads[base + k * LDS_MARCH_THREADS];
#pragma unroll
          for (int k = 0; k < LDS_MARCH_WIDE_BATCH; k++) {
            int j = 4 * (base + k * LDS_MARCH_THREADS);
            checksum += (got[k].x + got[k].y + got[k].z + got[k].w) & sum_mask;
            lds_march_compare(s, got[k].x, lds_march_pattern(rs, j) ^ inv, pass, j);
            lds_march_compare(s, got[k].y, lds_march_pattern(rs, j + 1) ^ inv, pass, j + 1);
            lds_march_compare(s, got[k].z, lds_march_pattern(rs, j + 2) ^ inv, pass, j + 2);
            lds_march_compare(s, got[k].w, lds_march_pattern(rs, j + 3) ^ inv, pass, j + 3);
          }
        }
      }
      __syncthreads();
    }
  }
  // Wave reduction, written out (see the wave_* helpers for why). -1 as
  // unsigned is the largest value, so an unsigned min picks the earliest pass,
  // then the lowest word among the lanes that failed in that pass
  unsigned first_pass = (unsigned)s.first_pass;
  for (int off = 32; off > 0; off >>= 1) {
    s.mismatched += __shfl_xor(s.mismatched, off);
    s.dropped |= (unsigned)__shfl_xor((int)s.dropped, off);
    s.raised |= (unsigned)__shfl_xor((int)s.raised, off);
    checksum += (unsigned)__shfl_xor((int)checksum, off);
    first_pass = min(first_pass, (unsigned)__shfl_xor((int)first_pass, off));
  }
  unsigned first_word = (unsigned)s.first_pass == first_pass ? (unsigned)s.first_word : 0xFFFFFFFFu;
  for (int off = 32; off > 0; off >>= 1)
    first_word = min(first_word, (unsigned)__shfl_xor((int)first_word, off));
  if (lane == 0)
    store_record8(records, wave, (int)place, s.mismatched, (int)first_pass, (int)first_word,
                  (int)s.dropped, (int)s.raised, (int)checksum, 0);
}

// One untimed warm-up launch, then one timed launch (warm_then_timed_ms).
// Returns (records [blocks*4, 8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> lds_march(long blocks, long rounds, long seed,
                                            long inject_block, long inject_word,
                                            long inject_pass, long inject_bit) {
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  // bounded run: a round of one workgroup measures ~51 us on an MI355X
  // (BENCHMARKS.md "LDS march"). The LDS instructions alone would need ~14 k
  // clocks, ~6 us (163840 B x 4 written at 64 B/clk, x 2 read at 128 and x 2
  // at 256 B/clk); the rest is the hash arithmetic of the pattern, with one
  // wave per SIMD to hide it. One workgroup per CU on 256 CUs then puts 2^20
  // block-rounds at ~0.2 s
  TORCH_CHECK(rounds <= (1L << 20) && blocks * rounds <= (1L << 20),
              "blocks*rounds must be <= 2^20");
  TORCH_CHECK(inject_block >= -1 && inject_block < blocks, "inject_block out of range");
  TORCH_CHECK(inject_word >= -1 && inject_word < LDS_MARCH_WORDS, "inject_word out of range");
  TORCH_CHECK(inject_pass >= -1 && inject_pass < rounds * 4, "inject_pass out of range");
  TORCH_CHECK(inject_bit >= 0 && inject_bit < 32, "inject_bit out of range");
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  const size_t need = LDS_MARCH_WORDS * sizeof(unsigned);
  TORCH_CHECK(prop.sharedMemPerBlock >= need, "lds_march needs ", need,
              " B of LDS per workgroup; this device offers ", prop.sharedMemPerBlock);
  auto records = zero_records(blocks * (LDS_MARCH_THREADS / 64), 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    hipLaunchKernelGGL(lds_march_kernel, dim3(blocks), dim3(LDS_MARCH_THREADS), 0, stream,
                       reinterpret_cast<int4*>(records.data_ptr<int>()), (int)rounds,
                       (unsigned)seed, (int)inject_block, (int)inject_word, (int)inject_pass,
                       (int)inject_bit);
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// VALU burn: a bounded, timed, exactly verifiable run of sustained vector-ALU
// issue on every SIMD, built like the MFMA burn-in above. Each lane carries
// one small state, seeded from (seed, section, lane) only, so every wave
// computes the same 64 values. Each round re-seeds the state, applies `chain`
// dependent steps and compares the state bitwise against expected[lane],
// which the host mirror (ops.valu_burn_expected) computes. The hot loop has
// no memory traffic. SEC selects what a step is made of:
//   int    v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32, add, xor, v_alignbit
//          rotate, v_bfe_u32, v_bcnt popcount
//   f32    v_cvt_f32_u32, v_ldexp_f32, the f32 FMA (emitted in its v_fmac_f32
//          encoding), v_pk_fma_f32, v_cvt_u32_f32
//   f64    v_cvt_f64_u32, the f64 FMA twice (v_fmac_f64), and v_trunc_f64,
//          v_ldexp_f64, v_floor_f64, v_cvt_u32_f64 on the way back
//   xlane  DPP quad_perm, row_shr and row_mirror, v_permlane32_swap,
//          ds_bpermute, v_readlane
//   trans  v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32, v_sin_f32
// Exactness by construction: the int and xlane steps are integer arithmetic
// and data movement. The f32 step multiplies two 12-bit integers and adds a
// 13-bit one, 4095*4095 + 8191 = 2^24, so every fma result is an integer that
// fp32 holds exactly; the power-of-two scaling around the scalar fma is exact
// and only moves the exponent path. The f64 step multiplies two 26-bit
// integers and adds one below 2^52: below 2^53, exact in fp64. So a
// pure-integer mirror reproduces these four sections bit for bit, whatever
// the rounding mode or evaluation order. (Checked in the gfx950 disassembly:
// each section's inner loop issues the instructions listed; BENCHMARKS.md
// "SIMD probe".)
//
// The trans section is different. The low bits of the transcendental unit's
// results are hardware-defined, so there is no host golden: `expected` is
// ignored, nothing is compared in the kernel, and the host checks consensus,
// every wave's checksum against the majority. It can name a SIMD that
// disagrees with the others; it CANNOT catch a fault common to all SIMDs.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word; the SIMD is HW_ID[5:4])
//   [1] mismatched lane-rounds
//   [2] first bad round (-1 if none)
//   [3] lowest bad lane in that round (-1 if none)
//   [4] [5] xor over lanes and rounds of the state, low and high word
//   [6] [7] 0 (reserved)
// Every round ends in the same state, so the xor over an even number of
// rounds cancels: a checksum says something for odd `rounds` only.
//
// inject_* (default -1 = off): in wave inject_wave, at round inject_round,
// lane inject_lane xors bit inject_bit into its state before the compare.
// Register arithmetic only, as in the MFMA burn-in.
// ---------------------------------------------------------------------------
enum { VALU_INT = 0, VALU_F32 = 1, VALU_F64 = 2, VALU_XLANE = 3, VALU_TRANS = 4 };
typedef __attribute__((ext_vector_type(2))) float f32x2;

// rotate left by k in [1,31] with v_alignbit_b32: ({x,x} >> (32-k))[31:0]
__device__ __forceinline__ unsigned rotl32(unsigned x, int k) {
  return __builtin_amdgcn_alignbit(x, x, 32 - k);
}

// low word: the u32 sections' state; both words: the f64 section's
__device__ __forceinline__ unsigned long long valu_seed_state(unsigned seed, int section,
                                                              int lane) {
  unsigned lo = fmix32(seed + (unsigned)section * 0x9E3779B9u + (unsigned)lane * 0x85EBCA6Bu);
  unsigned hi = fmix32(lo ^ 0xC2B2AE35u);
  return ((unsigned long long)hi << 32) | lo;
}

template <int SEC> struct ValuStep;

template <> struct ValuStep<VALU_INT> {
  typedef unsigned state;
  static __device__ __forceinline__ state step(state s, int lane, int c) {
    unsigned lo = s * 0x9E3779B1u;
    unsigned hi = __umulhi(s, 0x85EBCA6Bu);
    unsigned long long m = (unsigned long long)lo * (hi | 1u) + (((unsigned long long)hi << 32) | s);
    unsigned t = ((unsigned)m ^ (unsigned)(m >> 32)) + lo;
    return (rotl32(t, 13) ^ __builtin_amdgcn_ubfe(hi, 7, 11)) + (unsigned)__popc(lo);
  }
};

template <> struct ValuStep<VALU_F32> {
  typedef unsigned state;
  static __device__ __forceinline__ state step(state s, int lane, int c) {
    // a, b < 2^12 and c < 2^13: a*b + c <= 2^24, exact in fp32. The scalar
    // fma runs scaled by 2^k, k in [-8, 7], and is scaled back: exact too
    const int k = (int)((s >> 5) & 15u) - 8;
    float a = __builtin_amdgcn_ldexpf((float)(s & 0xFFFu), k);
    float b = (float)((s >> 12) & 0xFFFu);
    float cc = __builtin_amdgcn_ldexpf((float)(s >> 19), k);
    unsigned r0 = (unsigned)__builtin_amdgcn_ldexpf(__builtin_fmaf(a, b, cc), -k);
    f32x2 pa = {(float)((s >> 3) & 0xFFFu), (float)((s >> 9) & 0xFFFu)};
    f32x2 pb = {(float)((s >> 16) & 0xFFFu), (float)((s >> 1) & 0xFFFu)};
    f32x2 pc = {(float)((s >> 7) & 0x1FFFu), (float)((s >> 13) & 0x1FFFu)};
    f32x2 pr = __builtin_elementwise_fma(pa, pb, pc);
    unsigned r1 = (unsigned)pr.x, r2 = (unsigned)pr.y;
    return (s * 0x9E3779B1u + 0x7F4A7C15u) ^ (r0 + (r1 << 5) + (r2 << 9));
  }
};

template <> struct ValuStep<VALU_F64> {
  typedef unsigned long long state;
  static __device__ __forceinline__ state step(state s, int lane, int c) {
    // a, b, ch, cl < 2^26: cc = ch*2^26 + cl < 2^52 and a*b < 2^52, so
    // a*b + cc < 2^53: both fmas are exact in fp64
    const unsigned m26 = 0x3FFFFFFu;
    double a = (double)((unsigned)s & m26);
    double b = (double)((unsigned)(s >> 26) & m26);
    double cc = __builtin_fma((double)(unsigned)(s >> 38), 67108864.0,
                              (double)((unsigned)(s >> 7) & m26));
    unsigned long long r = (unsigned long long)__builtin_fma(a, b, cc);
    return (s * 0x9E3779B97F4A7C15ull + 0xBF58476D1CE4E5B9ull) ^ r ^ (r << 11);
  }
};

template <> struct ValuStep<VALU_XLANE> {
  typedef unsigned state;
  // old = src in every DPP move: a lane whose source is outside its row keeps
  // its own value
  template <int CTRL> static __device__ __forceinline__ unsigned dpp(unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xF, 0xF, false);
  }
  static __device__ __forceinline__ state step(state s, int lane, int c) {
    unsigned x = s;
    x = rotl32(x, 5) + dpp<0xB1>(x);    // quad_perm:[1,0,3,2]: lane l reads l^1
    x = rotl32(x, 7) ^ dpp<0x111>(x);   // row_shr:1: l reads l-1, l%16 == 0 itself
    x = x + rotl32(dpp<0x140>(x), 13);  // row_mirror: l reads l^15
    // vdst lanes 32-63 swap with src lanes 0-31; the other halves stay
    auto sw = __builtin_amdgcn_permlane32_swap(x, rotl32(x, 3), false, false);
    x = sw[0] + (sw[1] ^ 0x9E3779B9u);
    unsigned from = (unsigned)(lane * 13 + 7) & 63u;  // a bijection on the lanes
    x = rotl32(x, 9) ^ (unsigned)__builtin_amdgcn_ds_bpermute((int)(from << 2), (int)x);
    return x + (unsigned)__builtin_amdgcn_readlane((int)x, (c * 11 + 5) & 63);
  }
};

template <> struct ValuStep<VALU_TRANS> {
  typedef unsigned state;
  static __device__ __forceinline__ state step(state s, int lane, int c) {
    float f = __uint_as_float(0x3F800000u | (s & 0x7FFFFFu));  // [1, 2)
    unsigned e = __float_as_uint(__builtin_amdgcn_exp2f(f));
    unsigned l = __float_as_uint(__builtin_amdgcn_logf(f));
    unsigned rc = __float_as_uint(__builtin_amdgcn_rcpf(f));
    unsigned rq = __float_as_uint(__builtin_amdgcn_rsqf(f));
    unsigned sq = __float_as_uint(__builtin_amdgcn_sqrtf(f));
    unsigned sn = __float_as_uint(__builtin_amdgcn_sinf(f * 0.125f));  // argument in turns
    return (s * 0x9E3779B1u + 0x7F4A7C15u) ^ e ^ rotl32(l, 3) ^ rotl32(rc, 7) ^ rotl32(rq, 11) ^
           rotl32(sq, 17) ^ rotl32(sn, 23);
  }
};

template <int SEC>
__global__ void __launch_bounds__(256)
valu_burn_kernel(const long long* __restrict__ expected, int4* __restrict__ records,
                 unsigned seed, int chain, int rounds, int inject_wave, int inject_round,
                 int inject_lane, int inject_bit) {
  typedef ValuStep<SEC> V;
  typedef typename V::state state;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned place = hw_word();

  const state seeded = (state)valu_seed_state(seed, SEC, lane);
  state want = 0;
  if constexpr (SEC != VALU_TRANS) want = (state)expected[lane];
  const state flip =
      (wave == inject_wave && lane == inject_lane) ? (state)1 << (inject_bit & (int)(8 * sizeof(state) - 1)) : (state)0;
  int mismatched = 0, first_round = -1, first_lane = -1;
  state checksum = 0;
  for (int round = 0; round < rounds; round++) {
    state s = seeded;
    // opaque to the optimiser: every round really recomputes its chain
    asm volatile("" : "+v"(s));
    for (int c = 0; c < chain; c++) s = V::step(s, lane, c);
    if (round == inject_round) s ^= flip;
    checksum ^= s;
    if constexpr (SEC != VALU_TRANS) {
      const unsigned long long bad = __ballot(s != want);  // wave-uniform
      if (bad) {
        mismatched += __popcll(bad);
        if (first_round < 0) {
          first_round = round;
          first_lane = __ffsll((long long)bad) - 1;
        }
      }
    }
  }
  // wave reduction, written out (see the wave_* helpers for why)
  unsigned lo = (unsigned)checksum, hi = (unsigned)((unsigned long long)checksum >> 32);
  for (int off = 32; off > 0; off >>= 1) {
    lo ^= (unsigned)__shfl_xor((int)lo, off);
    hi ^= (unsigned)__shfl_xor((int)hi, off);
  }
  if (lane == 0)
    store_record8(records, wave, (int)place, mismatched, first_round, first_lane, (int)lo, (int)hi,
                  0, 0);
}

// ---------------------------------------------------------------------------
// VGPR march: a timed write/read-verify of a SIMD's vector register file in
// both bit polarities. VGPRs and AGPRs are one file of 512 entries per lane
// per SIMD (128 KiB per SIMD, 512 KiB per CU). This kernel allocates all 512
// (256 + 256), so its wave is the only one its SIMD can hold and owns the
// file; the host entry asserts that occupancy on every run.
//
// A pass is ONE asm statement: it writes v32..v255 and a0..a255 in ascending
// order, xors the two injection masks into one fixed VGPR and one fixed AGPR,
// then reads all of them back in ascending order and compares. The statement
// names every register it marches as a clobber (which also makes the kernel
// descriptor allocate 256 + 256); between statements the compiler is free to
// use them, so nothing of a pass may straddle two statements. v0..v31 are
// where the compiler keeps the kernel's own values and the statement's
// operands: 480 of the 512 entries are marched.
//
// Pattern: in round r register R (0..255 architectural, 256..511 the
// accumulators) of lane l holds
//   p(r, R, l) = ((R*64 + l) * 0x9E3779B1 mod 2^32) ^ rs,
//   rs = fmix32(seed + r*0x9E3779B9),
// then its complement in the round's second pass. Multiplication by an odd
// constant and xor with a constant are bijections on 32 bits, so the 32768
// values of a pass are distinct and an aliased register or lane reads back
// as wrong data. In the asm that is v_add_u32 v[R], (R*64*K) mod 2^32, l*K
// and v_xor_b32 with rs (or ~rs).
//
// Several hundred independent instructions separate a register's write from
// its read-back. Where a temporary is produced and consumed back to back
// around a v_accvgpr_* move it is padded with s_nop 1: that is a precaution,
// not a measured requirement.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched (register, lane) pairs over all passes
//   [2] first bad global pass, round*2 + polarity (-1 if none)
//   [3] lowest mismatching register index R in that pass (-1 if none)
//   [4] dropped mask: OR of (want & ~got), bits that should be 1 and read 0
//   [5] raised mask:  OR of (got & ~want), bits that should be 0 and read 1
//   [6] sum mod 2^32 of every value read in the pattern passes
//   [7] registers marched per pass (480)
//
// inject_* (default -1 = off): in wave inject_wave, at global pass
// inject_pass, lane inject_lane's mask for v[VGPR_MARCH_INJECT_V] (target 0)
// or a[VGPR_MARCH_INJECT_A] (target 1) holds bit inject_bit; everywhere else
// both masks are zero. They are xored in unconditionally, between the write
// and the read phase, inside the statement. Registers only.
// ---------------------------------------------------------------------------
constexpr int VGPR_MARCH_FIRST = 32;     // v0..v31 stay the compiler's
constexpr int VGPR_MARCH_MARCHED = 480;  // v32..v255 and a0..a255
constexpr int VGPR_MARCH_INJECT_V = 77;  // R = 77
constexpr int VGPR_MARCH_INJECT_A = 141; // R = 256 + 141 = 397

// compare the value in GOT against the pattern of register index R (both
// assembler expressions); t0 = want, t1 = diff, t2 = scratch. Plain VALU
// arithmetic on VGPRs only: no VCC or SGPR is written and read back, so no
// VALU-writes-SGPR wait states are owed inside the string. t2 = min(1, diff)
// is 1 on a mismatch; t2 - 1 is then 0 on a mismatch and all ones otherwise,
// and or-ing R into it leaves R or all ones for the running min
#define VGPR_MARCH_CHECK(GOT, R)                                        \
  "v_add_u32 %[t0], ((" R ")*64*0x9E3779B1)&0xffffffff, %[base]\n\t"    \
  "v_xor_b32 %[t0], %[xr], %[t0]\n\t"                                   \
  "v_xor_b32 %[t1], %[t0], " GOT "\n\t"                                 \
  "v_and_b32 %[t2], %[smask], " GOT "\n\t"                              \
  "v_add_u32 %[sum], %[sum], %[t2]\n\t"                                 \
  "v_and_or_b32 %[dropped], %[t0], %[t1], %[dropped]\n\t"               \
  "v_and_or_b32 %[raised], " GOT ", %[t1], %[raised]\n\t"               \
  "v_min_u32 %[t2], 1, %[t1]\n\t"                                       \
  "v_add_u32 %[mism], %[mism], %[t2]\n\t"                               \
  "v_add_u32 %[t2], -1, %[t2]\n\t"                                      \
  "v_or_b32 %[t2], " R ", %[t2]\n\t"                                    \
  "v_min_u32 %[first], %[first], %[t2]\n\t"

// the clobber list: "v32".."v255", "a0".."a255", ten names per HVD_C10
#define HVD_C10(P, d)                                                                  \
  P #d "0", P #d "1", P #d "2", P #d "3", P #d "4", P #d "5", P #d "6", P #d "7", P #d "8", \
      P #d "9"
#define HVD_C50(P, a, b, c, d, e) \
  HVD_C10(P, a), HVD_C10(P, b), HVD_C10(P, c), HVD_C10(P, d), HVD_C10(P, e)
#define HVD_C40_249(P)                                                                   \
  HVD_C10(P, 4), HVD_C50(P, 5, 6, 7, 8, 9), HVD_C50(P, 10, 11, 12, 13, 14),              \
      HVD_C50(P, 15, 16, 17, 18, 19), HVD_C50(P, 20, 21, 22, 23, 24), P "250", P "251", \
      P "252", P "253", P "254", P "255"
#define VGPR_MARCH_CLOBBERS                                                              \
  "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", HVD_C40_249("v"), "a0", "a1", \
      "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", HVD_C10("a", 1), HVD_C10("a", 2),  \
      HVD_C10("a", 3), HVD_C40_249("a")

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
vgpr_march_kernel(int4* __restrict__ records, int rounds, unsigned seed, int inject_wave,
                  int inject_target, int inject_lane, int inject_bit, int inject_pass) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned place = hw_word();

  const unsigned base = (unsigned)lane * 0x9E3779B1u;
  const unsigned flip =
      (wave == inject_wave && lane == inject_lane) ? 1u << (inject_bit & 31) : 0u;
  unsigned mism = 0, dropped = 0, raised = 0, sum = 0;
  int first_pass = -1;
  unsigned first_reg = 0xFFFFFFFFu;
#pragma nounroll
  for (int pass = 0; pass < 2 * rounds; pass++) {
    const unsigned rs = fmix32(seed + (unsigned)(pass >> 1) * 0x9E3779B9u);
    const unsigned xr = (pass & 1) ? ~rs : rs;            // wave-uniform
    const unsigned smask = (pass & 1) ? 0u : 0xFFFFFFFFu;  // sum pattern passes only
    const unsigned m0 = (pass == inject_pass && inject_target == 0) ? flip : 0u;
    const unsigned m1 = (pass == inject_pass && inject_target == 1) ? flip : 0u;
    unsigned first = 0xFFFFFFFFu, t0, t1, t2, t3;
    asm volatile(
        // write phase, architectural registers v32..v255
        ".set hvd_r, 32\n\t"
        ".rept 224\n\t"
        "v_add_u32 v[hvd_r], (hvd_r*64*0x9E3779B1)&0xffffffff, %[base]\n\t"
        "v_xor_b32 v[hvd_r], %[xr], v[hvd_r]\n\t"
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        // write phase, accumulators a0..a255 (R = 256..511)
        ".set hvd_r, 0\n\t"
        ".rept 256\n\t"
        "v_add_u32 %[t0], ((hvd_r+256)*64*0x9E3779B1)&0xffffffff, %[base]\n\t"
        "v_xor_b32 %[t0], %[xr], %[t0]\n\t"
        "s_nop 1\n\t"
        "v_accvgpr_write_b32 a[hvd_r], %[t0]\n\t"
        "s_nop 1\n\t"
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        // injection: masks are zero except in one wave, lane and pass
        "v_xor_b32 v77, %[m0], v77\n\t"
        "v_accvgpr_read_b32 %[t0], a141\n\t"
        "s_nop 1\n\t"
        "v_xor_b32 %[t0], %[m1], %[t0]\n\t"
        "s_nop 1\n\t"
        "v_accvgpr_write_b32 a141, %[t0]\n\t"
        "s_nop 1\n\t"
        // read phase, architectural registers
        ".set hvd_r, 32\n\t"
        ".rept 224\n\t"
        VGPR_MARCH_CHECK("v[hvd_r]", "hvd_r")
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        // read phase, accumulators
        ".set hvd_r, 0\n\t"
        ".rept 256\n\t"
        "v_accvgpr_read_b32 %[t3], a[hvd_r]\n\t"
        "s_nop 1\n\t"
        VGPR_MARCH_CHECK("%[t3]", "hvd_r+256")
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        : [mism] "+v"(mism), [dropped] "+v"(dropped), [raised] "+v"(raised), [sum] "+v"(sum),
          [first] "+v"(first), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [t3] "=&v"(t3)
        : [base] "v"(base), [xr] "s"(xr), [smask] "v"(smask), [m0] "v"(m0), [m1] "v"(m1)
        : VGPR_MARCH_CLOBBERS);
    const bool first_here = first != 0xFFFFFFFFu && first_pass < 0;
    first_pass = first_here ? pass : first_pass;
    first_reg = first_here ? first : first_reg;
  }
  // Wave reduction, written out (see the wave_* helpers for why): the earliest
  // pass by unsigned min (-1 is the largest value), then the lowest register
  // among the lanes that failed in that pass
  unsigned fp = (unsigned)first_pass;
  for (int off = 32; off > 0; off >>= 1) {
    mism += (unsigned)__shfl_xor((int)mism, off);
    dropped |= (unsigned)__shfl_xor((int)dropped, off);
    raised |= (unsigned)__shfl_xor((int)raised, off);
    sum += (unsigned)__shfl_xor((int)sum, off);
    fp = min(fp, (unsigned)__shfl_xor((int)fp, off));
  }
  unsigned fr = (unsigned)first_pass == fp ? first_reg : 0xFFFFFFFFu;
  for (int off = 32; off > 0; off >>= 1) fr = min(fr, (unsigned)__shfl_xor((int)fr, off));
  if (lane == 0)
    store_record8(records, wave, (int)place, (int)mism, (int)fp, (int)fr, (int)dropped,
                  (int)raised, (int)sum, VGPR_MARCH_MARCHED);
}

// expected: 64 int64 on the current device, the state every lane must reach
// after `chain` steps (ops.valu_burn_expected); section "trans" compares
// nothing and may pass an empty tensor. One untimed warm-up launch, then one
// timed launch (warm_then_timed_ms).
// Returns (records [waves,8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> valu_burn(torch::Tensor expected, const std::string& section,
                                            long seed, long blocks, long chain, long rounds,
                                            long inject_wave, long inject_round,
                                            long inject_lane, long inject_bit) {
  int sec = section == "int" ? VALU_INT : section == "f32" ? VALU_F32 : section == "f64" ? VALU_F64
            : section == "xlane" ? VALU_XLANE : section == "trans" ? VALU_TRANS : -1;
  TORCH_CHECK(sec >= 0, "section must be one of int, f32, f64, xlane, trans; got ", section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  // the checksum is all the trans section has, and over an even number of
  // (identical) rounds it is zero whatever the hardware computed
  TORCH_CHECK(sec != VALU_TRANS || rounds % 2 == 1,
              "section trans needs an odd number of rounds (its xor checksum cancels over an "
              "even number)");
  // bounded run: at most 2^22 steps per wave. At eight waves per SIMD the
  // slowest section (f32) measures ~0.5 us per step (BENCHMARKS.md "SIMD
  // probe"), ~2 s for 2^22 of them at the default grid
  TORCH_CHECK(chain <= (1L << 22) && rounds <= (1L << 22) && chain * rounds <= (1L << 22),
              "chain*rounds must be <= 2^22");
  const long state_bits = sec == VALU_F64 ? 64 : 32;
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds && inject_lane >= -1 && inject_lane < 64 &&
                  inject_bit >= -1 && inject_bit < state_bits,
              "inject_wave/inject_round/inject_lane/inject_bit out of range");
  TORCH_CHECK(inject_wave < 0 || (inject_round >= 0 && inject_lane >= 0 && inject_bit >= 0),
              "an injection needs inject_round, inject_lane and inject_bit");
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  const long long* want = nullptr;
  if (sec != VALU_TRANS || expected.numel() != 0) {
    TORCH_CHECK(expected.is_cuda() && expected.get_device() == dev,
                "expected must be on the current GPU");
    TORCH_CHECK(expected.dtype() == torch::kInt64 && expected.numel() == 64,
                "expected must hold 64 int64 values (one state per lane)");
    expected = expected.contiguous();
    want = reinterpret_cast<const long long*>(expected.data_ptr<int64_t>());
  }
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<5>(sec, [&](auto sec_c) {
      hipLaunchKernelGGL((valu_burn_kernel<decltype(sec_c)::value>), dim3(blocks), dim3(256), 0,
                         stream, want, reinterpret_cast<int4*>(records.data_ptr<int>()),
                         (unsigned)seed, (int)chain, (int)rounds, (int)inject_wave,
                         (int)inject_round, (int)inject_lane, (int)inject_bit);
    });
  });
  return std::make_tuple(records, ms);
}

// One untimed warm-up launch, then one timed launch (warm_then_timed_ms).
// Returns (records [blocks*4, 8] int32, elapsed_ms of the timed launch,
// resident workgroups per CU as the occupancy query reports them: always 1).
std::tuple<torch::Tensor, double, long> vgpr_march(long blocks, long rounds, long seed,
                                                   long inject_wave, long inject_target,
                                                   long inject_lane, long inject_bit,
                                                   long inject_pass) {
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  // bounded run: a round (two passes) of one workgroup measures ~34 us on an
  // MI355X (BENCHMARKS.md "SIMD probe"); one workgroup per CU on 256 CUs then
  // puts 2^20 block-rounds at ~0.14 s
  TORCH_CHECK(rounds <= (1L << 20) && blocks * rounds <= (1L << 20),
              "blocks*rounds must be <= 2^20");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4, "inject_wave out of range");
  TORCH_CHECK(inject_target == 0 || inject_target == 1, "inject_target must be 0 or 1");
  TORCH_CHECK(inject_lane >= 0 && inject_lane < 64, "inject_lane out of range");
  TORCH_CHECK(inject_bit >= 0 && inject_bit < 32, "inject_bit out of range");
  TORCH_CHECK(inject_pass >= -1 && inject_pass < rounds * 2, "inject_pass out of range");
  // the premise of the march, asserted on every run: a wave that holds all
  // 512 registers per lane is alone on its SIMD, so one 256-thread workgroup
  // is all a CU can hold
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vgpr_march_kernel, 256, 0));
  TORCH_CHECK(per_cu == 1, "vgpr_march needs exactly one resident workgroup per CU (one wave ",
              "per SIMD); the occupancy query reports ", per_cu);
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    hipLaunchKernelGGL(vgpr_march_kernel, dim3(blocks), dim3(256), 0, stream,
                       reinterpret_cast<int4*>(records.data_ptr<int>()), (int)rounds,
                       (unsigned)seed, (int)inject_wave, (int)inject_target, (int)inject_lane,
                       (int)inject_bit, (int)inject_pass);
  });
  return std::make_tuple(records, ms, (long)per_cu);
}

// ---------------------------------------------------------------------------
// Scalar probe, part 1. SALU burn: a bounded, timed, exactly verifiable run of
// sustained scalar-ALU issue, built like the VALU burn above. A CU has ONE
// scalar unit, shared by its four SIMDs; every kernel computes its
// wave-uniform addresses, loop counts, branch conditions and EXEC masks on it.
//
// Sections s32, s64 and ctl: each wave carries SALU_CHAINS = 8 independent
// states in SGPRs, seeded by valu_seed_state(seed, section, chain index), so
// every wave computes the same eight values. Each round re-seeds them, applies
// `chain` dependent steps to each and compares them on the SALU against
// expected[0..8), which the host mirror (ops.salu_burn_expected) computes. The
// steps are inline asm on "s" operands: in plain C++ the compiler chooses
// between SALU and VALU and folds constants. The state derives from kernel
// arguments and constants only, so it is wave-uniform for the compiler; the
// wave index is made so with readfirstlane. A 64-bit operand cannot be taken
// apart inside an asm string, so a step that needs the halves of one (the
// add/addc pair of s64, the s_cselect_b64 of ctl) is several statements with
// plain register-pair packing between them. What a step is made of:
//   s32   s_mul_i32, s_mul_hi_u32, s_mul_hi_i32, the carry chain s_add_u32 /
//         s_addc_u32 / s_sub_u32 / s_subb_u32, s_lshl/lshr_b32, s_ashr_i32,
//         s_bfe_u32/i32, s_bcnt1_i32_b32, s_ff1_i32_b32, s_flbit_i32_b32,
//         s_brev_b32, s_lshl{1,2,3,4}_add_u32, s_sext_i32_i8/i16,
//         s_absdiff_i32, s_min/max_{i,u}32, s_pack_{ll,lh,hh}_b32_b16,
//         s_bitset0/1_b32, s_andn2/orn2/nand/nor/xnor_b32
//   s64   s_lshl/lshr_b64, s_ashr_i64, s_bfe_u64/i64, a 64-bit add from
//         s_add_u32 + s_addc_u32, s_and/or/xor/andn2/nand/nor/xnor_b64,
//         s_not_b64, s_brev_b64, s_wqm_b64, s_bcnt1_i32_b64, s_ff1_i32_b64,
//         s_flbit_i32_b64, s_cmp_eq_u64 / s_cmp_lg_u64 into s_cselect_b32
//   ctl   SCC and control flow: s_movk_i32, s_mulk_i32, s_addk_i32, the twelve
//         s_cmp_{eq,lg,gt,ge,lt,le}_{i32,u32}, s_bitcmp0/1_b32 and the twelve
//         s_cmpk_*, each outcome shifted into a word with s_addc_u32 d, d, d;
//         s_cselect_b32/b64 and s_cmov_b32; then a data-dependent
//         s_cbranch_scc0 between two different updates and an s_cbranch_scc1
//         around a third (the mirror asserts that all four ways are taken)
// s_absdiff_i32 gets sign-extended 16- and 8-bit operands, so its difference
// cannot overflow; the bit-field extracts use constant fields inside the word.
// SCC is read only after a compare or an add/sub whose carry is defined.
//
// Section mask is where the scalar unit meets the vector unit, in plain C++
// (the compiler owns the VALU-writes-SGPR wait states): the state is per lane
// as in the VALU burn (expected[0..64)). A step ballots a state bit (v_cmp
// into an SGPR pair), takes the popcount and find-first of the mask on the
// SALU, updates the lanes inside and outside the mask by different formulas
// (EXEC saved, narrowed, inverted, restored) and feeds lane 0's value back
// through v_readfirstlane.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched chain-rounds (lane-rounds for mask)
//   [2] first bad round (-1 if none)
//   [3] lowest bad chain (lane) in that round (-1 if none)
//   [4] [5] xor over chains (lanes) and rounds of the state, low and high word
//   [6] [7] 0 (reserved)
// As in the VALU burn the checksum cancels over an even number of rounds.
//
// inject_* (default -1 = off): in wave inject_wave, at round inject_round,
// chain (lane) inject_chain has bit inject_bit xored into its state before the
// compare. Registers only.
//
// The scalar unit only READS memory in this probe (expected[], the pattern of
// part 3); everything it computes leaves the wave through store_record8, a
// vector store.
// ---------------------------------------------------------------------------
enum { SALU_S32 = 0, SALU_S64 = 1, SALU_CTL = 2, SALU_MASK = 3 };
constexpr int SALU_CHAINS = 8;

__device__ __forceinline__ unsigned long long u64_of(unsigned lo, unsigned hi) {
  return ((unsigned long long)hi << 32) | lo;
}

// A scalar load of N dwords and its wait, one asm statement with an early-clobber
// destination: scalar loads return out of order, and the compiler knows nothing
// of a load issued from asm. Part 3 below is built on these; the burn reads
// `expected` with one.
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(8))) unsigned u32x8;
typedef __attribute__((ext_vector_type(16))) unsigned u32x16;


// N dwords at byte offset byte_off (a multiple of 4*N), loaded and waited for
template <int N> struct ScalarLoad;
#define HVD_SCALAR_LOAD(N, T, MNEMONIC)                                                    \
  template <> struct ScalarLoad<N> {                                                       \
    typedef T vec;                                                                         \
    static __device__ __forceinline__ vec load(const int* p, unsigned byte_off) {          \
      vec v;                                                                               \
      asm volatile(MNEMONIC " %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"                          \
                   : "=&s"(v)                                                              \
                   : "s"(p), "s"(byte_off)                                                 \
                   : "memory");                                                            \
      return v;                                                                            \
    }                                                                                      \
  };
HVD_SCALAR_LOAD(2, u32x2, "s_load_dwordx2")
HVD_SCALAR_LOAD(4, u32x4, "s_load_dwordx4")
HVD_SCALAR_LOAD(8, u32x8, "s_load_dwordx8")
HVD_SCALAR_LOAD(16, u32x16, "s_load_dwordx16")
#undef HVD_SCALAR_LOAD
template <> struct ScalarLoad<1> {
  static __device__ __forceinline__ unsigned load(const int* p, unsigned byte_off) {
    unsigned v;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(v)
                 : "s"(p), "s"(byte_off)
                 : "memory");
    return v;
  }
};

template <int SEC> struct SaluStep;

template <> struct SaluStep<SALU_S32> {
  typedef unsigned state;
  static __device__ __forceinline__ state step(state s) {
    unsigned a, b, c, d, e, f;
    asm volatile(
        "s_mul_i32 %[a], %[s], 0x9E3779B1\n\t"
        "s_mul_hi_u32 %[b], %[s], 0x85EBCA6B\n\t"
        "s_mul_hi_i32 %[c], %[s], 0xC2B2AE35\n\t"
        "s_add_u32 %[a], %[a], %[b]\n\t"
        "s_addc_u32 %[b], %[b], %[c]\n\t"
        "s_sub_u32 %[c], %[c], %[a]\n\t"
        "s_subb_u32 %[a], %[a], %[b]\n\t"
        "s_addc_u32 %[c], %[c], %[s]\n\t"
        "s_lshl_b32 %[d], %[a], %[b]\n\t"
        "s_lshr_b32 %[e], %[c], %[a]\n\t"
        "s_xor_b32 %[d], %[d], %[e]\n\t"
        "s_ashr_i32 %[e], %[b], %[c]\n\t"
        "s_add_u32 %[d], %[d], %[e]\n\t"
        "s_bfe_u32 %[e], %[a], 0xB0007\n\t"
        "s_xor_b32 %[d], %[d], %[e]\n\t"
        "s_bfe_i32 %[e], %[c], 0xD0005\n\t"
        "s_add_u32 %[d], %[d], %[e]\n\t"
        "s_bcnt1_i32_b32 %[e], %[b]\n\t"
        "s_lshl1_add_u32 %[d], %[e], %[d]\n\t"
        "s_ff1_i32_b32 %[e], %[c]\n\t"
        "s_lshl2_add_u32 %[d], %[e], %[d]\n\t"
        "s_flbit_i32_b32 %[e], %[a]\n\t"
        "s_lshl3_add_u32 %[d], %[e], %[d]\n\t"
        "s_brev_b32 %[e], %[b]\n\t"
        "s_lshl4_add_u32 %[d], %[e], %[d]\n\t"
        "s_xor_b32 %[d], %[d], %[e]\n\t"
        "s_sext_i32_i16 %[e], %[a]\n\t"
        "s_sext_i32_i8 %[f], %[c]\n\t"
        "s_absdiff_i32 %[e], %[e], %[f]\n\t"
        "s_add_u32 %[d], %[d], %[e]\n\t"
        "s_min_i32 %[e], %[a], %[b]\n\t"
        "s_max_i32 %[f], %[a], %[c]\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        "s_min_u32 %[f], %[b], %[c]\n\t"
        "s_add_u32 %[e], %[e], %[f]\n\t"
        "s_max_u32 %[f], %[a], %[d]\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        "s_add_u32 %[d], %[d], %[e]\n\t"
        "s_pack_ll_b32_b16 %[e], %[a], %[b]\n\t"
        "s_pack_lh_b32_b16 %[f], %[b], %[c]\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        "s_pack_hh_b32_b16 %[f], %[c], %[a]\n\t"
        "s_add_u32 %[e], %[e], %[f]\n\t"
        "s_xor_b32 %[d], %[d], %[e]\n\t"
        "s_mov_b32 %[e], %[c]\n\t"
        "s_bitset0_b32 %[e], %[a]\n\t"
        "s_bitset1_b32 %[e], %[b]\n\t"
        "s_add_u32 %[d], %[d], %[e]\n\t"
        "s_andn2_b32 %[e], %[a], %[b]\n\t"
        "s_orn2_b32 %[f], %[b], %[c]\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        "s_nand_b32 %[f], %[c], %[a]\n\t"
        "s_add_u32 %[e], %[e], %[f]\n\t"
        "s_nor_b32 %[f], %[a], %[d]\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        "s_xnor_b32 %[f], %[b], %[d]\n\t"
        "s_add_u32 %[e], %[e], %[f]\n\t"
        "s_xor_b32 %[d], %[d], %[e]\n\t"
        "s_add_u32 %[s], %[d], 0x7F4A7C15\n\t"
        : [s] "+s"(s), [a] "=&s"(a), [b] "=&s"(b), [c] "=&s"(c), [d] "=&s"(d), [e] "=&s"(e),
          [f] "=&s"(f)
        :
        : "scc");
    return s;
  }
};

template <> struct SaluStep<SALU_S64> {
  typedef unsigned long long state;
  static __device__ __forceinline__ state step(state s) {
    unsigned long long A, B, C, D, E, F;
    asm volatile(
        "s_lshl_b64 %[A], %[s], 13\n\t"
        "s_lshr_b64 %[B], %[s], 7\n\t"
        "s_xor_b64 %[A], %[A], %[B]\n\t"
        "s_ashr_i64 %[B], %[s], 17\n\t"
        "s_xor_b64 %[A], %[A], %[B]\n\t"
        "s_bfe_u64 %[B], %[s], 0x280009\n\t"
        "s_bfe_i64 %[C], %[A], 0x1D0011\n\t"
        : [A] "=&s"(A), [B] "=&s"(B), [C] "=&s"(C)
        : [s] "s"(s)
        : "scc");
    // A += B, the 64-bit add of two register pairs
    unsigned alo = (unsigned)A, ahi = (unsigned)(A >> 32);
    asm volatile(
        "s_add_u32 %[alo], %[alo], %[blo]\n\t"
        "s_addc_u32 %[ahi], %[ahi], %[bhi]\n\t"
        : [alo] "+s"(alo), [ahi] "+s"(ahi)
        : [blo] "s"((unsigned)B), [bhi] "s"((unsigned)(B >> 32))
        : "scc");
    A = u64_of(alo, ahi);
    unsigned e, f, g, h;
    asm volatile(
        "s_and_b64 %[D], %[A], %[C]\n\t"
        "s_or_b64 %[E], %[B], %[C]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_andn2_b64 %[E], %[A], %[B]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_nand_b64 %[E], %[s], %[C]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_nor_b64 %[E], %[A], %[s]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_xnor_b64 %[E], %[B], %[s]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_not_b64 %[E], %[C]\n\t"
        "s_brev_b64 %[E], %[E]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_wqm_b64 %[E], %[B]\n\t"
        "s_xor_b64 %[D], %[D], %[E]\n\t"
        "s_bcnt1_i32_b64 %[e], %[A]\n\t"
        "s_ff1_i32_b64 %[f], %[D]\n\t"
        "s_flbit_i32_b64 %[g], %[C]\n\t"
        "s_bfe_u64 %[E], %[s], 0x10000\n\t"
        "s_bfe_u64 %[F], %[A], 0x10003\n\t"
        "s_cmp_eq_u64 %[E], %[F]\n\t"
        "s_cselect_b32 %[h], %[e], %[f]\n\t"
        "s_bfe_u64 %[F], %[B], 0x10005\n\t"
        "s_cmp_lg_u64 %[E], %[F]\n\t"
        "s_cselect_b32 %[g], %[g], %[e]\n\t"
        "s_lshl_b32 %[e], %[e], 8\n\t"
        "s_xor_b32 %[e], %[e], %[f]\n\t"
        : [D] "=&s"(D), [E] "=&s"(E), [F] "=&s"(F), [e] "=&s"(e), [f] "=&s"(f), [g] "=&s"(g),
          [h] "=&s"(h)
        : [s] "s"(s), [A] "s"(A), [B] "s"(B), [C] "s"(C)
        : "scc");
    unsigned dlo = (unsigned)D, dhi = (unsigned)(D >> 32);
    asm volatile(
        "s_add_u32 %[dlo], %[dlo], %[h]\n\t"
        "s_addc_u32 %[dhi], %[dhi], %[g]\n\t"
        "s_xor_b32 %[dhi], %[dhi], %[e]\n\t"
        "s_add_u32 %[dlo], %[dlo], 0x7F4A7C15\n\t"
        "s_addc_u32 %[dhi], %[dhi], 0x9E3779B9\n\t"
        : [dlo] "+s"(dlo), [dhi] "+s"(dhi)
        : [h] "s"(h), [g] "s"(g), [e] "s"(e)
        : "scc");
    return u64_of(dlo, dhi);
  }
};

template <> struct SaluStep<SALU_CTL> {
  typedef unsigned state;
  static __device__ __forceinline__ state step(state s) {
    unsigned a, b;
    asm volatile(
        "s_mov_b32 %[a], %[s]\n\t"
        "s_mulk_i32 %[a], 0x6b43\n\t"
        "s_addk_i32 %[a], 0x7c15\n\t"
        "s_lshr_b32 %[b], %[s], 15\n\t"
        "s_xor_b32 %[b], %[b], %[a]\n\t"
        : [a] "=&s"(a), [b] "=&s"(b)
        : [s] "s"(s)
        : "scc");
    const unsigned long long P = u64_of(b, a), Q = u64_of(s, b);
    unsigned long long R;
    unsigned n, c, d, e, f, g, h;
    // every compare's outcome goes into d as one bit: d = d + d + SCC
#define SALU_CTL_BIT "s_addc_u32 %[d], %[d], %[d]\n\t"
    asm volatile(
        "s_and_b32 %[c], %[a], 3\n\t"
        "s_and_b32 %[e], %[b], 3\n\t"
        "s_lshr_b32 %[g], %[a], 16\n\t"
        "s_lshr_b32 %[h], %[b], 16\n\t"
        "s_movk_i32 %[d], 0x1b\n\t"
        "s_movk_i32 %[f], -12059\n\t"
        "s_cmp_eq_i32 %[c], %[e]\n\t"
        "s_cselect_b32 %[n], %[a], %[b]\n\t" SALU_CTL_BIT
        "s_cmp_lg_i32 %[c], 2\n\t"
        "s_cmov_b32 %[f], %[h]\n\t" SALU_CTL_BIT
        "s_cmp_gt_i32 %[a], %[b]\n\t"
        "s_cselect_b64 %[R], %[P], %[Q]\n\t" SALU_CTL_BIT
        "s_cmp_ge_i32 %[b], %[s]\n\t" SALU_CTL_BIT
        "s_cmp_lt_i32 %[a], %[s]\n\t" SALU_CTL_BIT
        "s_cmp_le_i32 %[s], %[b]\n\t" SALU_CTL_BIT
        "s_cmp_eq_u32 %[e], 1\n\t" SALU_CTL_BIT
        "s_cmp_lg_u32 %[c], %[e]\n\t" SALU_CTL_BIT
        "s_cmp_gt_u32 %[a], %[b]\n\t" SALU_CTL_BIT
        "s_cmp_ge_u32 %[b], %[s]\n\t" SALU_CTL_BIT
        "s_cmp_lt_u32 %[s], %[a]\n\t" SALU_CTL_BIT
        "s_cmp_le_u32 %[h], %[g]\n\t" SALU_CTL_BIT
        "s_bitcmp0_b32 %[a], %[b]\n\t" SALU_CTL_BIT
        "s_bitcmp1_b32 %[b], %[a]\n\t" SALU_CTL_BIT
        "s_cmpk_eq_i32 %[c], 1\n\t" SALU_CTL_BIT
        "s_cmpk_lg_i32 %[e], 2\n\t" SALU_CTL_BIT
        "s_cmpk_gt_i32 %[a], 0x1234\n\t" SALU_CTL_BIT
        "s_cmpk_ge_i32 %[b], -4660\n\t" SALU_CTL_BIT
        "s_cmpk_lt_i32 %[a], -28672\n\t" SALU_CTL_BIT
        "s_cmpk_le_i32 %[b], 0x7000\n\t" SALU_CTL_BIT
        "s_cmpk_eq_u32 %[e], 3\n\t" SALU_CTL_BIT
        "s_cmpk_lg_u32 %[c], 0\n\t" SALU_CTL_BIT
        "s_cmpk_gt_u32 %[g], 0x8000\n\t" SALU_CTL_BIT
        "s_cmpk_ge_u32 %[h], 0x4000\n\t" SALU_CTL_BIT
        "s_cmpk_lt_u32 %[g], 0xc000\n\t" SALU_CTL_BIT
        "s_cmpk_le_u32 %[h], 0x2000\n\t" SALU_CTL_BIT
        "s_xor_b32 %[n], %[n], %[f]\n\t"
        // two different updates, chosen by a state bit
        "s_bitcmp1_b32 %[s], 7\n\t"
        "s_cbranch_scc0 hvd_ctl_else_%=\n\t"
        "s_mul_i32 %[n], %[n], 0x9E3779B1\n\t"
        "s_add_u32 %[n], %[n], %[d]\n\t"
        "s_branch hvd_ctl_join_%=\n"
        "hvd_ctl_else_%=:\n\t"
        "s_sub_u32 %[n], %[n], %[d]\n\t"
        "s_xor_b32 %[n], %[n], %[a]\n"
        "hvd_ctl_join_%=:\n\t"
        // a third, skipped when the new value is below b
        "s_cmp_lt_u32 %[n], %[b]\n\t"
        "s_cbranch_scc1 hvd_ctl_skip_%=\n\t"
        "s_not_b32 %[n], %[n]\n\t"
        "s_add_u32 %[n], %[n], %[h]\n"
        "hvd_ctl_skip_%=:\n\t"
        : [n] "=&s"(n), [c] "=&s"(c), [d] "=&s"(d), [e] "=&s"(e), [f] "=&s"(f), [g] "=&s"(g),
          [h] "=&s"(h), [R] "=&s"(R)
        : [s] "s"(s), [a] "s"(a), [b] "s"(b), [P] "s"(P), [Q] "s"(Q)
        : "scc");
#undef SALU_CTL_BIT
    asm volatile(
        "s_xor_b32 %[n], %[n], %[rlo]\n\t"
        "s_add_u32 %[n], %[n], %[rhi]\n\t"
        : [n] "+s"(n)
        : [rlo] "s"((unsigned)R), [rhi] "s"((unsigned)(R >> 32))
        : "scc");
    return n;
  }
};

// one step of the mask section for this lane; c is the step index
__device__ __forceinline__ unsigned salu_mask_step(unsigned s, int lane, int c) {
  const unsigned long long m = __ballot((s >> (c & 31)) & 1u);
  const unsigned pc = (unsigned)__popcll(m);
  const unsigned ff = (unsigned)__ffsll((long long)m);  // 0 for an empty mask, else 1 + index
  // the empty asm keeps the two arms a real branch on EXEC: without it the
  // compiler turns them into a select
  if ((m >> lane) & 1) {
    s = s * 0x9E3779B1u + pc;
    asm volatile("" : "+v"(s));
  } else {
    s = (s ^ (s >> 15)) * 0x85EBCA6Bu + ff;
    asm volatile("" : "+v"(s));
  }
  const unsigned first = (unsigned)__builtin_amdgcn_readfirstlane((int)s);
  return s + (first ^ (unsigned)m ^ (unsigned)(m >> 32));
}

// the wave index as a value the compiler knows to be wave-uniform
__device__ __forceinline__ int uniform_wave_index() {
  return (int)blockIdx.x * (int)(blockDim.x >> 6) +
         __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

template <int SEC>
__global__ void __launch_bounds__(256)
salu_burn_kernel(const long long* __restrict__ expected, int4* __restrict__ records,
                 unsigned seed, int chain, int rounds, int inject_wave, int inject_round,
                 int inject_chain, int inject_bit) {
  typedef SaluStep<SEC> S;
  typedef typename S::state state;
  const int wave = uniform_wave_index();
  const unsigned place = hw_word();

  const state flip =
      wave == inject_wave ? (state)1 << (inject_bit & (int)(8 * sizeof(state) - 1)) : (state)0;
  int mismatched = 0, first_round = -1, first_chain = -1;
  state checksum = 0;
  for (int round = 0; round < rounds; round++) {
    // Opaque to the optimiser: every round really recomputes its chains. The
    // seeds are derived again each round and the expected values loaded after
    // the chain loop, instead of both held in 32 more SGPRs across it (with
    // them the s64 section spilled)
    unsigned sd = seed;
    asm volatile("" : "+s"(sd));
    state s[SALU_CHAINS];
#pragma unroll
    for (int k = 0; k < SALU_CHAINS; k++) s[k] = (state)valu_seed_state(sd, SEC, k);
    for (int c = 0; c < chain; c++) {
#pragma unroll
      for (int k = 0; k < SALU_CHAINS; k++) s[k] = S::step(s[k]);
    }
    // expected[0..8) is 16 dwords: one scalar load. The compare is asm too, so
    // that it stays on the SALU; from the highest chain down, so that `low`
    // ends as the lowest bad one
    const u32x16 w = ScalarLoad<16>::load(reinterpret_cast<const int*>(expected), 0u);
    // masks, not selects: integer arithmetic on wave-uniform values stays on the SALU
    const state flip_now = flip & ((state)0 - (state)(round == inject_round));
    int bad = 0, low = -1;
#pragma unroll
    for (int k = SALU_CHAINS - 1; k >= 0; k--) {
      s[k] ^= flip_now & ((state)0 - (state)(k == inject_chain));
      checksum ^= s[k];
      const state want = (state)u64_of(w[2 * k], w[2 * k + 1]);
      if constexpr (sizeof(state) == 8) {
        asm volatile("s_cmp_lg_u64 %[got], %[want]\n\t"
                     "s_cselect_b32 %[low], %[k], %[low]\n\t"
                     "s_addc_u32 %[bad], %[bad], 0"
                     : [bad] "+s"(bad), [low] "+s"(low)
                     : [got] "s"(s[k]), [want] "s"(want), [k] "s"(k)
                     : "scc");
      } else {
        asm volatile("s_cmp_lg_u32 %[got], %[want]\n\t"
                     "s_cselect_b32 %[low], %[k], %[low]\n\t"
                     "s_addc_u32 %[bad], %[bad], 0"
                     : [bad] "+s"(bad), [low] "+s"(low)
                     : [got] "s"(s[k]), [want] "s"(want), [k] "s"(k)
                     : "scc");
      }
    }
    mismatched += bad;
    if (bad && first_round < 0) {
      first_round = round;
      first_chain = low;
    }
  }
  if ((threadIdx.x & 63) == 0)
    store_record8(records, wave, (int)place, mismatched, first_round, first_chain,
                  (int)(unsigned)checksum, (int)(unsigned)((unsigned long long)checksum >> 32), 0,
                  0);
}

__global__ void __launch_bounds__(256)
salu_mask_burn_kernel(const long long* __restrict__ expected, int4* __restrict__ records,
                      unsigned seed, int chain, int rounds, int inject_wave, int inject_round,
                      int inject_lane, int inject_bit) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned place = hw_word();

  const unsigned seeded = (unsigned)valu_seed_state(seed, SALU_MASK, lane);
  const unsigned want = (unsigned)expected[lane];
  const unsigned flip = (wave == inject_wave && lane == inject_lane) ? 1u << (inject_bit & 31) : 0u;
  int mismatched = 0, first_round = -1, first_lane = -1;
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    unsigned s = seeded;
    asm volatile("" : "+v"(s));
    for (int c = 0; c < chain; c++) s = salu_mask_step(s, lane, c);
    if (round == inject_round) s ^= flip;
    checksum ^= s;
    const unsigned long long bad = __ballot(s != want);  // wave-uniform
    if (bad) {
      mismatched += __popcll(bad);
      if (first_round < 0) {
        first_round = round;
        first_lane = __ffsll((long long)bad) - 1;
      }
    }
  }
  checksum = wave_xor(checksum);
  if (lane == 0)
    store_record8(records, wave, (int)place, mismatched, first_round, first_lane, (int)checksum, 0,
                  0, 0);
}

// ---------------------------------------------------------------------------
// Scalar probe, part 2. SGPR march: a timed write/read-verify of the scalar
// registers a wave is given, in both bit polarities, built like the VGPR march
// above. A pass is ONE asm statement: it writes s32..s101 in ascending order,
// xors the injection mask into s77, then reads all of them back in ascending
// order and compares on the SALU. The statement names every register it
// marches as a clobber; s0..s31 stay the compiler's, for the kernel's own
// values and the statement's operands.
//
// Unlike the VGPR march this kernel CANNOT own the file. The SGPR file has 800
// entries per SIMD and a wave gets its allocation, not the file: the kernel
// verifies the 70 registers each wave was given, and the host sizes the grid
// so that the waves resident on a SIMD together hold most of the file.
//
// Pattern: in round r register R of global wave w holds
//   p(r, R, w) = ((w*128 + R) * 0x9E3779B1 mod 2^32) ^ rs,
//   rs = fmix32(seed + r*0x9E3779B9),
// then its complement in the round's second pass. The multiply by an odd
// constant is a bijection, so the values are distinct across the registers of
// a wave and across all waves of a launch (w < 2^25): co-resident waves hold
// different data, and an allocation that aliases another's reads back wrong.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched registers over all passes
//   [2] first bad global pass, round*2 + polarity (-1 if none)
//   [3] lowest mismatching register in that pass (-1 if none)
//   [4] dropped mask: OR of (want & ~got)   [5] raised mask: OR of (got & ~want)
//   [6] sum mod 2^32 of every value read in the pattern passes
//   [7] registers marched per pass (70)
//
// inject_* (default -1 = off): in wave inject_wave, at global pass
// inject_pass, the mask xored into s77 between the write and the read phase
// holds bit inject_bit; everywhere else it is zero. Registers only.
// ---------------------------------------------------------------------------
constexpr int SGPR_MARCH_FIRST = 32;    // s0..s31 stay the compiler's
constexpr int SGPR_MARCH_MARCHED = 70;  // s32..s101
constexpr int SGPR_MARCH_INJECT = 77;

#define SGPR_MARCH_CLOBBERS                                                               \
  "s32", "s33", "s34", "s35", "s36", "s37", "s38", "s39", HVD_C10("s", 4), HVD_C50("s", 5, 6, 7, \
                                                                                   8, 9),  \
      "s100", "s101"

__global__ void __launch_bounds__(256)
sgpr_march_kernel(int4* __restrict__ records, int rounds, unsigned seed, int inject_wave,
                  int inject_bit, int inject_pass) {
  const int wave = uniform_wave_index();
  const unsigned place = hw_word();

  const unsigned base = (unsigned)wave * 128u * 0x9E3779B1u;
  const unsigned flip = wave == inject_wave ? 1u << (inject_bit & 31) : 0u;
  unsigned mism = 0, dropped = 0, raised = 0, sum = 0;
  int first_pass = -1;
  unsigned first_reg = 0xFFFFFFFFu;
#pragma nounroll
  for (int pass = 0; pass < 2 * rounds; pass++) {
    const unsigned rs = fmix32(seed + (unsigned)(pass >> 1) * 0x9E3779B9u);
    // plain integer arithmetic, which stays on the SALU: selects of these
    // wave-uniform values have been seen to land in VGPRs
    const unsigned smask = (unsigned)(pass & 1) - 1u;  // all ones in pattern passes: sum those
    const unsigned xr = rs ^ ~smask;                   // the complement in the second pass
    const unsigned m = flip & (0u - (unsigned)(pass == inject_pass));
    unsigned first = 0xFFFFFFFFu, t0, t1, t2;
    asm volatile(
        // write phase
        ".set hvd_r, 32\n\t"
        ".rept 70\n\t"
        "s_add_u32 s[hvd_r], %[base], (hvd_r*0x9E3779B1)&0xffffffff\n\t"
        "s_xor_b32 s[hvd_r], s[hvd_r], %[xr]\n\t"
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        // injection: the mask is zero except in one wave and pass
        "s_xor_b32 s77, s77, %[m]\n\t"
        // read phase: t0 = want, t1 = diff
        ".set hvd_r, 32\n\t"
        ".rept 70\n\t"
        "s_add_u32 %[t0], %[base], (hvd_r*0x9E3779B1)&0xffffffff\n\t"
        "s_xor_b32 %[t0], %[t0], %[xr]\n\t"
        "s_and_b32 %[t2], s[hvd_r], %[smask]\n\t"
        "s_add_u32 %[sum], %[sum], %[t2]\n\t"
        "s_xor_b32 %[t1], %[t0], s[hvd_r]\n\t"
        "s_and_b32 %[t2], %[t0], %[t1]\n\t"
        "s_or_b32 %[dropped], %[dropped], %[t2]\n\t"
        "s_and_b32 %[t2], s[hvd_r], %[t1]\n\t"
        "s_or_b32 %[raised], %[raised], %[t2]\n\t"
        "s_cmp_lg_u32 %[t1], 0\n\t"
        "s_cselect_b32 %[t2], hvd_r, -1\n\t"
        "s_addc_u32 %[mism], %[mism], 0\n\t"
        "s_min_u32 %[first], %[first], %[t2]\n\t"
        ".set hvd_r, hvd_r+1\n\t"
        ".endr\n\t"
        : [mism] "+s"(mism), [dropped] "+s"(dropped), [raised] "+s"(raised), [sum] "+s"(sum),
          [first] "+s"(first), [t0] "=&s"(t0), [t1] "=&s"(t1), [t2] "=&s"(t2)
        : [base] "s"(base), [xr] "s"(xr), [smask] "s"(smask), [m] "s"(m)
        : "scc", SGPR_MARCH_CLOBBERS);
    const bool first_here = first != 0xFFFFFFFFu && first_pass < 0;
    first_pass = first_here ? pass : first_pass;
    first_reg = first_here ? first : first_reg;
  }
  if ((threadIdx.x & 63) == 0)
    store_record8(records, wave, (int)place, (int)mism, first_pass, (int)first_reg, (int)dropped,
                  (int)raised, (int)sum, SGPR_MARCH_MARCHED);
}

// ---------------------------------------------------------------------------
// Scalar probe, part 3. Scalar-load check: every wave reads a whole uint32
// pattern [2, W] (row 1 the complement of row 0) through the scalar data cache
// with s_load_dword, x2, x4, x8 and x16, one width per round, rotating, at
// offsets aligned to the load's own size, and compares every word on the SALU
// against the value recomputed from (seed, row, index):
//   row 0 word i = fmix32(seed ^ (i * 0x85EBCA6B)).
// The load and its s_waitcnt lgkmcnt(0) are one asm statement with an
// early-clobber destination: scalar loads return out of order, and the
// compiler knows nothing of a load issued from asm.
//
// This verifies the data bits of the scalar load path in both polarities and
// that all five widths return the right words. It does NOT march the scalar
// cache's cells: nothing lets a kernel choose them.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched words over all rounds
//   [2] first bad round (-1 if none)
//   [3] lowest bad word in that round, row*W + index (-1 if none)
//   [4] dropped mask   [5] raised mask
//   [6] sum mod 2^32 of the row-0 words read
//   [7] words read per round (2*W)
// There is no injection: a test flips a bit in the tensor it uploads.
// ---------------------------------------------------------------------------
struct ScalarLoadState {
  unsigned mismatched, first_word, dropped, raised, sum;
};

// Compare one loaded word on the SALU. j is its index within its row, idx its
// index in the buffer (row*W + j), inv all ones in row 1 (the complement) and
// smask all ones in row 0 (the row that is summed). One asm statement, so that
// the recomputed value, the compare and the bookkeeping stay scalar
// instructions: written in C++ the compiler moved them to the vector ALU.
// t = want, u = diff, w = scratch
__device__ __forceinline__ void scalar_load_compare(ScalarLoadState& s, unsigned got, unsigned seed,
                                                    unsigned j, unsigned idx, unsigned inv,
                                                    unsigned smask) {
  unsigned t, u, w;
  asm volatile(
      "s_mul_i32 %[t], %[j], 0x85EBCA6B\n\t"
      "s_xor_b32 %[t], %[t], %[seed]\n\t"
      // fmix32
      "s_lshr_b32 %[u], %[t], 16\n\t"
      "s_xor_b32 %[t], %[t], %[u]\n\t"
      "s_mul_i32 %[t], %[t], 0x85EBCA6B\n\t"
      "s_lshr_b32 %[u], %[t], 13\n\t"
      "s_xor_b32 %[t], %[t], %[u]\n\t"
      "s_mul_i32 %[t], %[t], 0xC2B2AE35\n\t"
      "s_lshr_b32 %[u], %[t], 16\n\t"
      "s_xor_b32 %[t], %[t], %[u]\n\t"
      "s_xor_b32 %[t], %[t], %[inv]\n\t"
      "s_and_b32 %[w], %[got], %[smask]\n\t"
      "s_add_u32 %[sum], %[sum], %[w]\n\t"
      "s_and_b32 %[w], %[t], %[got]\n\t"
      "s_xor_b32 %[w], %[w], %[t]\n\t"  // want & ~got
      "s_or_b32 %[dropped], %[dropped], %[w]\n\t"
      "s_and_b32 %[w], %[t], %[got]\n\t"
      "s_xor_b32 %[w], %[w], %[got]\n\t"  // got & ~want
      "s_or_b32 %[raised], %[raised], %[w]\n\t"
      "s_xor_b32 %[u], %[t], %[got]\n\t"  // SCC = mismatch
      "s_cselect_b32 %[w], %[idx], -1\n\t"
      "s_addc_u32 %[mism], %[mism], 0\n\t"
      "s_min_u32 %[first], %[first], %[w]\n\t"
      : [mism] "+s"(s.mismatched), [first] "+s"(s.first_word), [dropped] "+s"(s.dropped),
        [raised] "+s"(s.raised), [sum] "+s"(s.sum), [t] "=&s"(t), [u] "=&s"(u), [w] "=&s"(w)
      : [got] "s"(got), [seed] "s"(seed), [j] "s"(j), [idx] "s"(idx), [inv] "s"(inv),
        [smask] "s"(smask)
      : "scc");
}

// one row of the buffer (words dwords, a multiple of 16) through loads of N
// dwords. The row is a template argument so that inv and smask are constants:
// derived from a compare of the loop index they landed in VGPRs
template <int N, int ROW>
__device__ __forceinline__ void scalar_load_row(ScalarLoadState& s, const int* p, unsigned seed,
                                                unsigned words) {
  constexpr unsigned inv = ROW ? 0xFFFFFFFFu : 0u;
  const unsigned row_base = ROW ? words : 0u;
  for (unsigned j = 0; j < words; j += N) {
    const unsigned idx = row_base + j;
    if constexpr (N == 1) {
      scalar_load_compare(s, ScalarLoad<1>::load(p, idx * 4), seed, j, idx, inv, ~inv);
    } else {
      const typename ScalarLoad<N>::vec v = ScalarLoad<N>::load(p, idx * 4);
#pragma unroll
      for (int k = 0; k < N; k++) scalar_load_compare(s, v[k], seed, j + k, idx + k, inv, ~inv);
    }
  }
}

// one round: the whole buffer, row 0 then row 1
template <int N>
__device__ __forceinline__ void scalar_load_round(ScalarLoadState& s, const int* p, unsigned seed,
                                                  unsigned words) {
  scalar_load_row<N, 0>(s, p, seed, words);
  scalar_load_row<N, 1>(s, p, seed, words);
}

__global__ void __launch_bounds__(256)
scalar_load_kernel(const int* __restrict__ pattern, int4* __restrict__ records, unsigned seed,
                   int words, int rounds) {
  const int wave = uniform_wave_index();
  const unsigned place = hw_word();
  ScalarLoadState total = {0u, 0xFFFFFFFFu, 0u, 0u, 0u};
  int first_round = -1;
  for (int round = 0; round < rounds; round++) {
    ScalarLoadState s = {0u, 0xFFFFFFFFu, 0u, 0u, 0u};
    switch (round % 5) {
      case 0: scalar_load_round<1>(s, pattern, seed, (unsigned)words); break;
      case 1: scalar_load_round<2>(s, pattern, seed, (unsigned)words); break;
      case 2: scalar_load_round<4>(s, pattern, seed, (unsigned)words); break;
      case 3: scalar_load_round<8>(s, pattern, seed, (unsigned)words); break;
      default: scalar_load_round<16>(s, pattern, seed, (unsigned)words); break;
    }
    total.mismatched += s.mismatched;
    total.dropped |= s.dropped;
    total.raised |= s.raised;
    total.sum += s.sum;
    if (s.mismatched && first_round < 0) {
      first_round = round;
      total.first_word = s.first_word;
    }
  }
  if ((threadIdx.x & 63) == 0)
    store_record8(records, wave, (int)place, (int)total.mismatched, first_round,
                  (int)total.first_word, (int)total.dropped, (int)total.raised, (int)total.sum,
                  2 * words);
}

// expected: int64 on the current device, the states a wave must reach after
// `chain` steps (ops.salu_burn_expected): SALU_CHAINS values for sections s32,
// s64 and ctl, 64 (one per lane) for mask. One untimed warm-up launch, then
// one timed launch (warm_then_timed_ms).
// Returns (records [waves,8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> salu_burn(torch::Tensor expected, const std::string& section,
                                            long seed, long blocks, long chain, long rounds,
                                            long inject_wave, long inject_round,
                                            long inject_chain, long inject_bit) {
  int sec = section == "s32" ? SALU_S32 : section == "s64" ? SALU_S64 : section == "ctl" ? SALU_CTL
            : section == "mask" ? SALU_MASK : -1;
  TORCH_CHECK(sec >= 0, "section must be one of s32, s64, ctl, mask; got ", section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  // bounded run: at most 2^18 steps per chain per wave. At eight waves per
  // SIMD a step of all eight chains of the slowest section (ctl) measures
  // ~8.4 us (BENCHMARKS.md "Scalar probe"), ~2.2 s for 2^18 of them at the
  // default grid
  TORCH_CHECK(chain <= (1L << 18) && rounds <= (1L << 18) && chain * rounds <= (1L << 18),
              "chain*rounds must be <= 2^18");
  const long units = sec == SALU_MASK ? 64 : SALU_CHAINS;
  const long state_bits = sec == SALU_S64 ? 64 : 32;
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds && inject_chain >= -1 && inject_chain < units &&
                  inject_bit >= -1 && inject_bit < state_bits,
              "inject_wave/inject_round/inject_chain/inject_bit out of range");
  TORCH_CHECK(inject_wave < 0 || (inject_round >= 0 && inject_chain >= 0 && inject_bit >= 0),
              "an injection needs inject_round, inject_chain and inject_bit");
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  TORCH_CHECK(expected.is_cuda() && expected.get_device() == dev,
              "expected must be on the current GPU");
  TORCH_CHECK(expected.dtype() == torch::kInt64 && expected.numel() == units,
              "expected must hold ", units, " int64 values for section ", section);
  expected = expected.contiguous();
  const long long* want = reinterpret_cast<const long long*>(expected.data_ptr<int64_t>());
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, want,
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (unsigned)seed,
                         (int)chain, (int)rounds, (int)inject_wave, (int)inject_round,
                         (int)inject_chain, (int)inject_bit);
    };
    if (sec == SALU_MASK) {
      launch(salu_mask_burn_kernel);
    } else {
      dispatch_int<3>(sec, [&](auto sec_c) { launch(salu_burn_kernel<decltype(sec_c)::value>); });
    }
  });
  return std::make_tuple(records, ms);
}

// One untimed warm-up launch, then one timed launch (warm_then_timed_ms).
// Returns (records [blocks*4, 8] int32, elapsed_ms of the timed launch, waves
// per SIMD as the occupancy query reports them: reported, never asserted, for
// the query over-reports for SGPR-heavy 256-thread kernels).
std::tuple<torch::Tensor, double, long> sgpr_march(long blocks, long rounds, long seed,
                                                   long inject_wave, long inject_bit,
                                                   long inject_pass) {
  // the pattern is unique across waves while w*128 + R < 2^32: w < 2^25
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  // bounded run: a round (two passes) measures ~3.7 us per workgroup on a CU
  // (BENCHMARKS.md "Scalar probe"); on 256 CUs that puts 2^27 block-rounds at
  // ~2 s
  TORCH_CHECK(rounds <= (1L << 27) && blocks * rounds <= (1L << 27),
              "blocks*rounds must be <= 2^27");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4, "inject_wave out of range");
  TORCH_CHECK(inject_bit >= 0 && inject_bit < 32, "inject_bit out of range");
  TORCH_CHECK(inject_pass >= -1 && inject_pass < rounds * 2, "inject_pass out of range");
  int per_cu = 0;
  HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sgpr_march_kernel, 256, 0));
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    hipLaunchKernelGGL(sgpr_march_kernel, dim3(blocks), dim3(256), 0, stream,
                       reinterpret_cast<int4*>(records.data_ptr<int>()), (int)rounds,
                       (unsigned)seed, (int)inject_wave, (int)inject_bit, (int)inject_pass);
  });
  // a 256-thread workgroup is one wave on each of the four SIMDs
  return std::make_tuple(records, ms, (long)per_cu);
}

// pattern: int32 [2, W] on the current device (ops.scalar_load_pattern viewed
// as int32), W a multiple of 16 in [16, 4096]. One untimed warm-up launch,
// then one timed launch (warm_then_timed_ms).
// Returns (records [blocks*4, 8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> scalar_load_check(torch::Tensor pattern, long seed, long blocks,
                                                    long rounds) {
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  TORCH_CHECK(pattern.is_cuda() && pattern.get_device() == dev,
              "pattern must be on the current GPU");
  TORCH_CHECK(pattern.dtype() == torch::kInt32, "pattern must be int32");
  TORCH_CHECK(pattern.dim() == 2 && pattern.size(0) == 2, "pattern must be [2, W]");
  const long words = pattern.size(1);
  TORCH_CHECK(words >= 16 && words <= 4096 && words % 16 == 0,
              "W must be a multiple of 16 in [16, 4096]; got ", words);
  TORCH_CHECK(pattern.is_contiguous(), "pattern must be contiguous");
  // bounded run: 2048 workgroups x 5 rounds x 1024 words measure ~3.7 ms
  // (BENCHMARKS.md "Scalar probe"), ~0.35 ns per workgroup-round-word: ~1.5 s
  // for 2^32 of them
  TORCH_CHECK(rounds <= (1L << 24) && blocks * rounds * words <= (1L << 32),
              "blocks*rounds*W must be <= 2^32");
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    hipLaunchKernelGGL(scalar_load_kernel, dim3(blocks), dim3(256), 0, stream,
                       pattern.data_ptr<int>(), reinterpret_cast<int4*>(records.data_ptr<int>()),
                       (unsigned)seed, (int)words, (int)rounds);
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// xGMI p2p bandwidth between two devices (one direction).
// ---------------------------------------------------------------------------
double p2p_gbps(int src_dev, int dst_dev, long size_mb, long iters) {
  TORCH_CHECK(size_mb > 0 && iters > 0);
  long bytes = size_mb * 1024 * 1024;
  int canAccess = 0;
  HIP_CHECK(hipDeviceCanAccessPeer(&canAccess, dst_dev, src_dev));
  DeviceAllocs src_buf, dst_buf;  // one per device: below, each is freed under its own
  HIP_CHECK(hipSetDevice(src_dev));
  void* src = src_buf.alloc(bytes);
  HIP_CHECK(hipSetDevice(dst_dev));
  void* dst = dst_buf.alloc(bytes);
  if (canAccess) {
    HIP_CHECK(hipSetDevice(dst_dev));
    hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
    TORCH_CHECK(e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled,
                "enable peer access failed: ", hipGetErrorString(e));
  }
  HIP_CHECK(hipSetDevice(src_dev));
  OwnedStream stream;
  HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream.s));  // warmup
  const double ms = timed_ms(stream.s, [&]() {
    for (long i = 0; i < iters; i++) {
      HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, stream.s));
    }
  });
  stream.destroy();
  src_buf.free_all();
  HIP_CHECK(hipSetDevice(dst_dev));
  dst_buf.free_all();
  HIP_CHECK(hipSetDevice(src_dev));
  double sec = ms / 1e3;
  return (double)bytes * iters / sec / 1e9;
}

// ---------------------------------------------------------------------------
// HBM pattern sweep: stuck-bit / corruption scan over a bounded span of HBM.
// Writes an address-derived 64-bit pattern, reads it back after the full
// write pass (chunk >> L2, so read-back hits HBM), counts mismatches with a
// device-side atomic. Catches data-integrity faults that bandwidth tests
// (triad) cannot see. Memory-bounded: one chunk allocated at a time with
// plain hipMalloc; allocation failure ends the sweep gracefully.
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {
  // splitmix64 finalizer: full-period, all 64 bits participate
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ void pattern_write_kernel(unsigned long long* __restrict__ p, long n,
                                     unsigned long long seed) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = mix64(seed ^ (unsigned long long)i);
}

__global__ void pattern_verify_kernel(const unsigned long long* __restrict__ p, long n,
                                      unsigned long long seed,
                                      unsigned long long* __restrict__ errors) {
  long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  unsigned long long local = 0;
  for (; i < n; i += stride)
    if (p[i] != mix64(seed ^ (unsigned long long)i)) local++;
  if (local) atomicAdd(errors, local);
}

// Sweep up to max_gib GiB of this device's HBM in chunk_gib chunks. All
// chunks are HELD until the sweep ends: a free/alloc loop would get the same
// physical block back each time and re-scan one region. Coverage is bounded
// by free memory minus headroom; allocation failure ends the sweep
// gracefully (bytes_tested reports actual coverage).
// Returns {bytes_tested, errors, write_gbps, verify_gbps}.
py::dict hbm_sweep(long max_gib, long chunk_gib, long seed) {
  TORCH_CHECK(max_gib > 0 && chunk_gib > 0 && chunk_gib <= max_gib);
  const long chunk_bytes = chunk_gib << 30;
  const long n = chunk_bytes / 8;
  size_t freeB = 0, totalB = 0;
  HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
  const long headroom = 8L << 30;
  long budget = std::min(max_gib << 30, (long)freeB - headroom);
  DeviceAllocs counter, chunks;
  unsigned long long* errs_d =
      static_cast<unsigned long long*>(counter.alloc_zeroed(sizeof(unsigned long long)));
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  double write_s = 0, verify_s = 0;
  long tested = 0;
  int blocks = 8192, threads = 256;  // >> 256 CUs, fills all 8 XCDs
  for (long off = 0; off + chunk_bytes <= budget; off += chunk_bytes) {
    unsigned long long* p = static_cast<unsigned long long*>(chunks.alloc(chunk_bytes, false));
    if (p == nullptr) break;
    unsigned long long chunk_seed = (unsigned long long)seed ^ (unsigned long long)off;
    write_s += timed_ms(stream, [&]() {
      hipLaunchKernelGGL(pattern_write_kernel, dim3(blocks), dim3(threads), 0, stream, p, n,
                         chunk_seed);
    }) / 1e3;
    verify_s += timed_ms(stream, [&]() {
      hipLaunchKernelGGL(pattern_verify_kernel, dim3(blocks), dim3(threads), 0, stream, p, n,
                         chunk_seed, errs_d);
    }) / 1e3;
    tested += chunk_bytes;
  }
  chunks.free_all();
  unsigned long long errs = 0;
  HIP_CHECK(hipMemcpy(&errs, errs_d, sizeof(errs), hipMemcpyDeviceToHost));
  counter.free_all();
  py::dict d;
  d["bytes_tested"] = (long long)tested;
  d["errors"] = (long long)errs;
  d["write_gbps"] = write_s > 0 ? tested / write_s / 1e9 : 0.0;
  d["verify_gbps"] = verify_s > 0 ? tested / verify_s / 1e9 : 0.0;
  // A busy tenant GPU can leave < headroom + one chunk free, so the loop
  // never runs; a zero-byte sweep is NOT evidence of health and callers
  // (gpu_health_report) must not count it as a pass.
  d["skipped"] = (bool)(tested == 0);
  return d;
}

// ---------------------------------------------------------------------------
// HBM march: a timed write/read-verify of a bounded span of HBM in both bit
// polarities through the widest access path, with the location, bits and
// direction of any mismatch recorded, and with each workgroup's XCD and
// realtime-clock span recorded so the host can give a bandwidth per XCD.
// hbm_sweep above returns one error count from one polarity through 8-byte
// accesses, and seeds every chunk separately.
//
// Pattern: p(seed, g) = mix64(seed ^ g), g the GLOBAL qword index in the whole
// sweep (chunk byte offset / 8 + index inside the chunk). For a fixed seed
// mix64(seed ^ .) is a bijection on 64 bits, so all values of a sweep are
// distinct and an address-decoder alias inside or across chunks reads back as
// a data mismatch. Pass 0 writes p, pass 1 writes ~p; each write launch is
// followed by a verify launch of its own (the kernel boundary provides the
// visibility; no workgroup waits for another).
//
// Geometry: a tile is 16 KiB = 256 threads x 16 B x 4 accesses; in access k
// thread t touches the 16 B at tile_base + (k*256 + t)*16, so each wave
// instruction covers 1 KiB contiguous. Workgroup b handles tiles b, b+blocks,
// b+2*blocks, ... of the chunk: a static assignment, so a slow XCD finishes
// late instead of handing its work to a fast one. Chunks are a multiple of
// 16 KiB, so there is no tail. All index arithmetic is 64-bit.
//
// Checked in the gfx950 disassembly: the write loop issues four
// global_store_dwordx4 per tile, the verify loop four global_load_dwordx4
// (all four issued before the first compare), the records leave as
// global_store_dwordx4, and wall_clock64() is s_memrealtime (100 MHz).
//
// Per-workgroup record, 16 x int32, four int4 vector stores by thread 0 after
// a shuffle reduction per wave and a four-entry LDS reduction across waves
// (a workgroup that received no tile still writes one):
//   [0]      placement word of wave 0 (hw_word)
//   [1]      tiles this workgroup processed
//   [2],[3]  realtime clock before the first access, lo / hi
//   [4],[5]  realtime clock after the last access has completed and the
//            workgroup has passed a barrier, lo / hi
//   verify only (the write kernel leaves these 0):
//   [6],[7]   mismatched qwords, lo / hi
//   [8],[9]   lowest mismatching global qword index, lo / hi (-1,-1 if none)
//   [10],[11] dropped mask: OR of (want & ~got)
//   [12],[13] raised mask:  OR of (got & ~want)
//   [14],[15] sum mod 2^64 of every qword read
//
// Bad-location log: [max_log, 4] int64 rows {global qword index, pass, want,
// got} plus a device counter. A thread appends at most one row per launch, for
// its first mismatch: it takes a slot with atomicAdd and writes only if the
// slot is < max_log, so a wholly broken chunk costs at most blocks x 256
// atomics per launch. The order is not deterministic; the host sorts.
//
// hbm_march_poke_kernel: one thread xors one bit of one qword of the sweep's
// own allocation, launched on the same stream between the write and the
// verify launch of one pass. A plain store that sends a known one-bit fault
// through the real verify path on healthy hardware.
// ---------------------------------------------------------------------------
constexpr int HBM_MARCH_THREADS = 256;
constexpr int HBM_MARCH_ACCESSES = 4;
constexpr long HBM_MARCH_TILE_BYTES = 16384;
constexpr long HBM_MARCH_TILE_QWORDS = HBM_MARCH_TILE_BYTES / 8;
constexpr long HBM_MARCH_TILE_VECS = HBM_MARCH_TILE_BYTES / 16;
static_assert(HBM_MARCH_THREADS * 16 * HBM_MARCH_ACCESSES == HBM_MARCH_TILE_BYTES,
              "a tile is threads x 16 B x accesses");
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ int4 hbm_march_pair(unsigned long long a, unsigned long long b) {
  return make_int4((int)(unsigned)a, (int)(unsigned)(a >> 32), (int)(unsigned)b,
                   (int)(unsigned)(b >> 32));
}

__global__ void __launch_bounds__(HBM_MARCH_THREADS)
hbm_march_write_kernel(u32x4* __restrict__ p, unsigned long long chunk_qword_base, long tiles,
                       unsigned long long seed, int invert, int4* __restrict__ records) {
  const int t = threadIdx.x;
  const unsigned place = hw_word();
  const unsigned long long inv = invert ? ~0ull : 0ull;
  const unsigned long long start = wall_clock64();
  asm volatile("" ::: "memory");
  int done = 0;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    u32x4* tp = p + tile * HBM_MARCH_TILE_VECS + t;
    const unsigned long long g0 =
        chunk_qword_base + (unsigned long long)tile * HBM_MARCH_TILE_QWORDS + 2ull * t;
    u32x4 val[HBM_MARCH_ACCESSES];
#pragma unroll
    for (int k = 0; k < HBM_MARCH_ACCESSES; k++) {
      const unsigned long long g = g0 + 2ull * k * HBM_MARCH_THREADS;
      const unsigned long long a = mix64(seed ^ g) ^ inv;
      const unsigned long long b = mix64(seed ^ (g + 1)) ^ inv;
      val[k] = (u32x4){(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
    }
#pragma unroll
    for (int k = 0; k < HBM_MARCH_ACCESSES; k++) tp[k * HBM_MARCH_THREADS] = val[k];
    done++;
  }
  // every wave waits for its own stores, then the barrier: past it, all of the
  // workgroup's stores have completed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned long long end = wall_clock64();
  if (t == 0) {
    int4* rec = records + 4 * (long)blockIdx.x;
    rec[0] = make_int4((int)place, done, (int)(unsigned)start,
                       (int)(unsigned)(start >> 32));
    // the empty asm keeps each a global_store_dwordx4 of its own: the compiler
    // otherwise regroups the constant words across the four stores
    asm volatile("" ::: "memory");
    rec[1] = make_int4((int)(unsigned)end, (int)(unsigned)(end >> 32), 0, 0);
    asm volatile("" ::: "memory");
    rec[2] = make_int4(0, 0, 0, 0);
    asm volatile("" ::: "memory");
    rec[3] = make_int4(0, 0, 0, 0);
  }
}

struct HbmMarchState {
  unsigned long long mismatched, first, dropped, raised, sum;
};

// a thread visits its qwords in ascending global order, so the first mismatch
// it sees in a launch is its lowest
__device__ __forceinline__ void hbm_march_compare(HbmMarchState& s, unsigned long long got,
                                                  unsigned long long want, unsigned long long g,
                                                  int pass, long long* __restrict__ log,
                                                  unsigned long long* __restrict__ log_count,
                                                  int max_log) {
  s.sum += got;
  const unsigned long long diff = got ^ want;
  if (diff != 0) {  // not taken on healthy memory
    if (s.mismatched == 0) {
      s.first = g;
      const unsigned long long slot = atomicAdd(log_count, 1ull);
      if (slot < (unsigned long long)max_log) {
        long long* row = log + 4 * slot;
        row[0] = (long long)g;
        row[1] = pass;
        row[2] = (long long)want;
        row[3] = (long long)got;
      }
    }
    s.mismatched++;
    s.dropped |= want & diff;
    s.raised |= got & diff;
  }
}

__global__ void __launch_bounds__(HBM_MARCH_THREADS)
hbm_march_verify_kernel(const u32x4* __restrict__ p, unsigned long long chunk_qword_base,
                        long tiles, unsigned long long seed, int invert, int pass,
                        int4* __restrict__ records, long long* __restrict__ log,
                        unsigned long long* __restrict__ log_count, int max_log) {
  __shared__ unsigned long long red[HBM_MARCH_THREADS / 64][5];
  const int t = threadIdx.x;
  const unsigned place = hw_word();
  const unsigned long long inv = invert ? ~0ull : 0ull;
  HbmMarchState s = {0ull, ~0ull, 0ull, 0ull, 0ull};
  const unsigned long long start = wall_clock64();
  asm volatile("" ::: "memory");
  int done = 0;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u32x4* tp = p + tile * HBM_MARCH_TILE_VECS + t;
    const unsigned long long g0 =
        chunk_qword_base + (unsigned long long)tile * HBM_MARCH_TILE_QWORDS + 2ull * t;
    // all four loads of the tile are in flight before the first compare
    u32x4 got[HBM_MARCH_ACCESSES];
#pragma unroll
    for (int k = 0; k < HBM_MARCH_ACCESSES; k++) got[k] = tp[k * HBM_MARCH_THREADS];
#pragma unroll
    for (int k = 0; k < HBM_MARCH_ACCESSES; k++) {
      const unsigned long long g = g0 + 2ull * k * HBM_MARCH_THREADS;
      const unsigned long long a = ((unsigned long long)got[k].y << 32) | got[k].x;
      const unsigned long long b = ((unsigned long long)got[k].w << 32) | got[k].z;
      hbm_march_compare(s, a, mix64(seed ^ g) ^ inv, g, pass, log, log_count, max_log);
      hbm_march_compare(s, b, mix64(seed ^ (g + 1)) ^ inv, g + 1, pass, log, log_count, max_log);
    }
    done++;
  }
  // the compares consumed every load, so the last access has completed here
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const unsigned long long end = wall_clock64();
  // opaque to the scheduler: the reduction stays behind the clock read
  asm volatile("" : "+v"(s.mismatched), "+v"(s.first), "+v"(s.dropped), "+v"(s.raised),
               "+v"(s.sum));
  s.mismatched = wave_add(s.mismatched);
  s.first = wave_min(s.first);
  s.dropped = wave_or(s.dropped);
  s.raised = wave_or(s.raised);
  s.sum = wave_add(s.sum);
  if ((t & 63) == 0) {
    unsigned long long* r = red[t >> 6];
    r[0] = s.mismatched;
    r[1] = s.first;
    r[2] = s.dropped;
    r[3] = s.raised;
    r[4] = s.sum;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < HBM_MARCH_THREADS / 64; w++) {
      s.mismatched += red[w][0];
      s.first = min(s.first, red[w][1]);
      s.dropped |= red[w][2];
      s.raised |= red[w][3];
      s.sum += red[w][4];
    }
    int4* rec = records + 4 * (long)blockIdx.x;
    rec[0] = make_int4((int)place, done, (int)(unsigned)start,
                       (int)(unsigned)(start >> 32));
    asm volatile("" ::: "memory");  // four stores, as in the write kernel
    rec[1] = make_int4((int)(unsigned)end, (int)(unsigned)(end >> 32), (int)(unsigned)s.mismatched,
                       (int)(unsigned)(s.mismatched >> 32));
    asm volatile("" ::: "memory");
    rec[2] = hbm_march_pair(s.first, s.dropped);
    asm volatile("" ::: "memory");
    rec[3] = hbm_march_pair(s.raised, s.sum);
  }
}

__global__ void hbm_march_poke_kernel(unsigned long long* __restrict__ p, long index, int bit) {
  if (blockIdx.x == 0 && threadIdx.x == 0) p[index] ^= 1ull << bit;
}

// March up to max_bytes of this device's HBM in chunks of chunk_bytes. Like
// hbm_sweep, chunks come from plain hipMalloc and are all HELD until the end
// (a free/alloc loop would get the same physical block back), the budget is
// min(max_bytes, free - 8 GiB headroom), and an allocation failure ends the
// march quietly. The headroom applies only above 1 GiB, so small shapes run on
// a busy card. Per chunk four launches run in order (write p, verify, write
// ~p, verify: pass 0 and pass 1), each timed on its own (timed_ms).
// Returns {records int32 [launches, blocks, 16] in launch order, elapsed_ms
// float64 [launches], log int64 [min(log_count, max_log), 4], log_count,
// bytes_tested, chunk_bytes, chunks, skipped}; the tensors are on the host.
py::dict hbm_march(long max_bytes, long chunk_bytes, long seed, long blocks, long max_log,
                   long inject_index, long inject_pass, long inject_bit) {
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  TORCH_CHECK(max_bytes > 0 && max_bytes <= (1L << 40), "max_bytes must be in [1, 2^40]");
  TORCH_CHECK(chunk_bytes > 0 && chunk_bytes % HBM_MARCH_TILE_BYTES == 0 &&
                  chunk_bytes <= max_bytes,
              "chunk_bytes must be a positive multiple of 16384 and <= max_bytes");
  TORCH_CHECK(max_log >= 0 && max_log <= (1L << 16), "max_log must be in [0, 2^16]");
  TORCH_CHECK(inject_index >= -1 && inject_index < max_bytes / 8, "inject_index out of range");
  TORCH_CHECK(inject_pass >= -1 && inject_pass <= 1, "inject_pass out of range");
  TORCH_CHECK(inject_bit >= 0 && inject_bit <= 63, "inject_bit out of range");
  size_t freeB = 0, totalB = 0;
  HIP_CHECK(hipMemGetInfo(&freeB, &totalB));
  const long headroom = max_bytes > (1L << 30) ? (8L << 30) : 0;
  const long budget = std::min(max_bytes, (long)freeB - headroom);
  const long tiles = chunk_bytes / HBM_MARCH_TILE_BYTES;
  const long chunk_qwords = chunk_bytes / 8;
  const size_t record_bytes = (size_t)blocks * 16 * sizeof(int);

  DeviceAllocs hold;  // freed when the march ends, also when a HIP_CHECK throws
  int4* records_d = static_cast<int4*>(hold.alloc_zeroed(record_bytes));
  long long* log_d =
      static_cast<long long*>(hold.alloc_zeroed((size_t)std::max(max_log, 1L) * 32));
  unsigned long long* count_d = static_cast<unsigned long long*>(hold.alloc_zeroed(8));
  HIP_CHECK(hipDeviceSynchronize());  // the memsets ran on the legacy stream
  hipStream_t stream = at::cuda::getCurrentCUDAStream();

  std::vector<int> records_h;
  std::vector<double> elapsed_h;
  // one timed launch; its records are copied out once timed_ms has waited for
  // the stop event
  auto timed = [&](auto&& launch) {
    elapsed_h.push_back(timed_ms(stream, launch));
    const size_t at = records_h.size();
    records_h.resize(at + (size_t)blocks * 16);
    HIP_CHECK(hipMemcpy(records_h.data() + at, records_d, record_bytes, hipMemcpyDeviceToHost));
  };

  long tested = 0, chunks = 0;
  for (long off = 0; off + chunk_bytes <= budget; off += chunk_bytes) {
    void* chunk = hold.alloc(chunk_bytes, false);
    if (chunk == nullptr) break;
    u32x4* p = static_cast<u32x4*>(chunk);
    const unsigned long long base = (unsigned long long)(off / 8);
    const long local = inject_index - off / 8;
    const bool inject_here = inject_index >= 0 && local >= 0 && local < chunk_qwords;
    for (int pass = 0; pass < 2; pass++) {
      timed([&]() {
        hipLaunchKernelGGL(hbm_march_write_kernel, dim3(blocks), dim3(HBM_MARCH_THREADS), 0,
                           stream, p, base, tiles, (unsigned long long)seed, pass, records_d);
      });
      if (inject_here && pass == inject_pass) {
        hipLaunchKernelGGL(hbm_march_poke_kernel, dim3(1), dim3(64), 0, stream,
                           static_cast<unsigned long long*>(chunk), local, (int)inject_bit);
        HIP_CHECK(hipGetLastError());
      }
      timed([&]() {
        hipLaunchKernelGGL(hbm_march_verify_kernel, dim3(blocks), dim3(HBM_MARCH_THREADS), 0,
                           stream, p, base, tiles, (unsigned long long)seed, pass, pass,
                           records_d, log_d, count_d, (int)max_log);
      });
    }
    tested += chunk_bytes;
    chunks++;
  }
  unsigned long long log_count = 0;
  HIP_CHECK(hipMemcpy(&log_count, count_d, sizeof(log_count), hipMemcpyDeviceToHost));
  const long rows = (long)std::min<unsigned long long>(log_count, (unsigned long long)max_log);
  auto log = torch::empty({rows, 4}, torch::TensorOptions().dtype(torch::kInt64));
  if (rows > 0)
    HIP_CHECK(hipMemcpy(log.data_ptr<int64_t>(), log_d, (size_t)rows * 32, hipMemcpyDeviceToHost));
  const long launches = (long)elapsed_h.size();
  auto records = torch::empty({launches, blocks, 16}, torch::TensorOptions().dtype(torch::kInt32));
  if (launches > 0)
    std::memcpy(records.data_ptr<int>(), records_h.data(), records_h.size() * sizeof(int));
  auto elapsed = torch::empty({launches}, torch::TensorOptions().dtype(torch::kFloat64));
  if (launches > 0)
    std::memcpy(elapsed.data_ptr<double>(), elapsed_h.data(), elapsed_h.size() * sizeof(double));
  py::dict d;
  d["records"] = records;
  d["elapsed_ms"] = elapsed;
  d["log"] = log;
  d["log_count"] = (long long)log_count;
  d["bytes_tested"] = (long long)tested;
  d["chunk_bytes"] = (long long)chunk_bytes;
  d["chunks"] = (long long)chunks;
  // as for hbm_sweep: a zero-byte march is not evidence of health
  d["skipped"] = (bool)(tested == 0);
  return d;
}

// ---------------------------------------------------------------------------
// Atomic probe, part 1: the exact atomic burn (ops.atomic_burn).
//
// Every lane owns its cells; cell j of lane l of a wave sits at element
// j*64 + l of the wave's region, so one wave-instruction touches 256 (4-byte
// cells) or 512 (8-byte cells) contiguous bytes. Cells are seeded from (seed,
// section, cell, lane) only: every wave computes the same thing. A step issues
// the section's fixed sequence of atomics, each operation once returning and
// once non-returning (result unused: the compiler selects the no-return
// instruction), with operands hashed from the lane's register mirror of the
// cell, the step and the operation. Every returned old value is compared with
// the mirror, which the VALU then advances; after the chain the cells are read
// back with relaxed atomic loads and compared with `expected`, the host
// mirror's final values (ops.atomic_burn_expected).
//
// Integer cells (sections g32, g64 and the u32 cells of lds), by what survives
// a wrong value: cell 0 add, sub, xor (bijective in the cell: a difference
// stays to the end of the round); cell 1 smin, smax, umin, umax; cell 2 and,
// or, swap; cell 3 inc, dec, cmpswap with the true value (must succeed),
// cmpswap with a wrong value (must fail and leave the cell alone).
// Float cells (section gfp and the float cells of lds): add f32, add f64,
// min / max f64, pk_add f16, pk_add bf16 on integers small enough that every
// sum is exact (ops.atomic_fp_exact proves it per seed and chain).
// Section lds runs the same on per-lane LDS cells, plus a u64 cell (add, xor),
// plus once per launch a ticket: all 256 lanes of the workgroup draw `chain`
// tickets from one LDS word and mark owner[ticket]; after a barrier the
// workgroup counts the unmarked entries and checks the word.
//
// No wave waits for another; every loop bound is a launch argument; a ticket
// is range-checked before it indexes. Operation index within a step: 2*k for
// the returning, 2*k + 1 for the non-returning form of the k-th operation in
// the order above (lds: integer cells, then the u64 cell, then the float
// cells); the index after the last one stands for the final compare.
//
// Record per wave: {hw word, mismatches (lane-steps, the final compare counting
// as one more step), first bad round (-1), lowest bad lane in it (-1),
// checksum lo, checksum hi (xor of the final cell values over lanes and
// rounds), that lane's first bad operation index (-1), ticket faults (lds:
// unmarked entries + out-of-range tickets + 1 if the word is not 256*chain)}.
//
// inject_* (default -1 = off): in wave inject_wave, at round inject_round, lane
// inject_lane issues one extra atomic xor of bit inject_bit on its own first
// cell before the chain: memory really differs from the mirror.
// ---------------------------------------------------------------------------
enum { ATOMIC_G32 = 0, ATOMIC_G64 = 1, ATOMIC_GFP = 2, ATOMIC_LDS = 3 };
enum { ATOMIC_INT_OPS = 28, ATOMIC_U64_OPS = 4, ATOMIC_FP_OPS = 12 };
enum { ATOMIC_FP_BYTES = 1792, ATOMIC_LDS_WAVE_BYTES = 512 + 1024 + ATOMIC_FP_BYTES };
enum { ATOMIC_LDS_MAX_CHAIN = 64 };  // owner[256 * chain] as u16: 32 KiB
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef short bf16x2 __attribute__((ext_vector_type(2)));

struct AtomicLaneCheck {
  int bad = 0;        // this step returned a wrong old value
  int first_op = -1;  // first wrong operation of this round
  __device__ __forceinline__ void see(bool wrong, int op) {
    if (wrong) {
      bad = 1;
      if (first_op < 0) first_op = op;
    }
  }
};

__device__ __forceinline__ unsigned atomic_operand(unsigned m, unsigned c, int i) {
  return fmix32(m ^ (c * 0x9E3779B1u + (unsigned)i * 0x85EBCA6Bu));
}
__device__ __forceinline__ unsigned long long atomic_operand(unsigned long long m, unsigned c,
                                                             int i) {
  return mix64(m ^ (unsigned long long)(c * 0x9E3779B1u + (unsigned)i * 0x85EBCA6Bu));
}

// the integer atomics on T (unsigned or unsigned long long) and what each does
// to the mirror
template <typename T, int SCOPE> struct AtomicInt {
  typedef typename std::make_signed<T>::type S;
  static __device__ __forceinline__ T add(T* p, T x) {
    return __hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T sub(T* p, T x) {
    return __hip_atomic_fetch_sub(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T xor_(T* p, T x) {
    return __hip_atomic_fetch_xor(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T and_(T* p, T x) {
    return __hip_atomic_fetch_and(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T or_(T* p, T x) {
    return __hip_atomic_fetch_or(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T umin(T* p, T x) {
    return __hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T umax(T* p, T x) {
    return __hip_atomic_fetch_max(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T smin(T* p, T x) {
    return (T)__hip_atomic_fetch_min(reinterpret_cast<S*>(p), (S)x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T smax(T* p, T x) {
    return (T)__hip_atomic_fetch_max(reinterpret_cast<S*>(p), (S)x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T swap(T* p, T x) {
    return __hip_atomic_exchange(p, x, __ATOMIC_RELAXED, SCOPE);
  }
  static __device__ __forceinline__ T inc(T* p, T x) {
    if constexpr (sizeof(T) == 4) {
      if constexpr (SCOPE == __HIP_MEMORY_SCOPE_AGENT)
        return __builtin_amdgcn_atomic_inc32(p, x, __ATOMIC_RELAXED, "agent");
      else
        return __builtin_amdgcn_atomic_inc32(p, x, __ATOMIC_RELAXED, "workgroup");
    } else {
      return __builtin_amdgcn_atomic_inc64(reinterpret_cast<unsigned long*>(p), x,
                                           __ATOMIC_RELAXED, "agent");
    }
  }
  static __device__ __forceinline__ T dec(T* p, T x) {
    if constexpr (sizeof(T) == 4) {
      if constexpr (SCOPE == __HIP_MEMORY_SCOPE_AGENT)
        return __builtin_amdgcn_atomic_dec32(p, x, __ATOMIC_RELAXED, "agent");
      else
        return __builtin_amdgcn_atomic_dec32(p, x, __ATOMIC_RELAXED, "workgroup");
    } else {
      return __builtin_amdgcn_atomic_dec64(reinterpret_cast<unsigned long*>(p), x,
                                           __ATOMIC_RELAXED, "agent");
    }
  }
  // the old value; the cell becomes x when it held cmp
  static __device__ __forceinline__ T cas(T* p, T cmp, T x) {
    __hip_atomic_compare_exchange_strong(p, &cmp, x, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return cmp;
  }
  static __device__ __forceinline__ T m_smin(T m, T x) { return (S)x < (S)m ? x : m; }
  static __device__ __forceinline__ T m_smax(T m, T x) { return (S)x > (S)m ? x : m; }
  static __device__ __forceinline__ T m_inc(T m, T x) { return m >= x ? (T)0 : m + 1; }
  static __device__ __forceinline__ T m_dec(T m, T x) { return (m == 0 || m > x) ? x : m - 1; }
};

// operation K on cell J: returning (compared), then non-returning
#define HVD_ATOMIC_PAIR(K, J, FETCH, APPLY)                       \
  x = atomic_operand(m[J], c, 2 * (K));                           \
  old = A::FETCH(p[J], x);                                        \
  chk.see(old != m[J], op_base + 2 * (K));                        \
  m[J] = APPLY;                                                   \
  x = atomic_operand(m[J], c, 2 * (K) + 1);                       \
  (void)A::FETCH(p[J], x);                                        \
  m[J] = APPLY;

template <typename T, int SCOPE> struct AtomicIntLane {
  typedef AtomicInt<T, SCOPE> A;
  T* p[4];
  T m[4];
  __device__ __forceinline__ void init(unsigned char* wave_base, int lane) {
#pragma unroll
    for (int j = 0; j < 4; j++) p[j] = reinterpret_cast<T*>(wave_base) + j * 64 + lane;
  }
  __device__ __forceinline__ void seed(unsigned sd, int sec, int lane) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      m[j] = (T)valu_seed_state(sd, sec, j * 64 + lane);
      __hip_atomic_store(p[j], m[j], __ATOMIC_RELAXED, SCOPE);
    }
  }
  __device__ __forceinline__ void inject(int bit) {
    (void)A::xor_(p[0], (T)1 << bit);
  }
  __device__ __forceinline__ void step(unsigned c, AtomicLaneCheck& chk, int op_base) {
    T x, old;
    HVD_ATOMIC_PAIR(0, 0, add, m[0] + x)
    HVD_ATOMIC_PAIR(1, 0, sub, m[0] - x)
    HVD_ATOMIC_PAIR(2, 0, xor_, m[0] ^ x)
    HVD_ATOMIC_PAIR(3, 1, smin, A::m_smin(m[1], x))
    HVD_ATOMIC_PAIR(4, 1, smax, A::m_smax(m[1], x))
    HVD_ATOMIC_PAIR(5, 1, umin, (x < m[1] ? x : m[1]))
    HVD_ATOMIC_PAIR(6, 1, umax, (x > m[1] ? x : m[1]))
    HVD_ATOMIC_PAIR(7, 2, and_, m[2] & x)
    HVD_ATOMIC_PAIR(8, 2, or_, m[2] | x)
    HVD_ATOMIC_PAIR(9, 2, swap, x)
    HVD_ATOMIC_PAIR(10, 3, inc, A::m_inc(m[3], x))
    HVD_ATOMIC_PAIR(11, 3, dec, A::m_dec(m[3], x))
    // cmpswap, true value: succeeds
    x = atomic_operand(m[3], c, 24);
    old = A::cas(p[3], m[3], x);
    chk.see(old != m[3], op_base + 24);
    m[3] = x;
    x = atomic_operand(m[3], c, 25);
    (void)A::cas(p[3], m[3], x);
    m[3] = x;
    // cmpswap, wrong value (differs in bit 0 at least): fails, cell untouched
    x = atomic_operand(m[3], c, 26);
    old = A::cas(p[3], m[3] ^ (x | 1), x);
    chk.see(old != m[3], op_base + 26);
    x = atomic_operand(m[3], c, 27);
    (void)A::cas(p[3], m[3] ^ (x | 1), x);
  }
  // expected: this group's cell 0, lane 0
  __device__ __forceinline__ bool wrong_final(const long long* expected, int lane,
                                              unsigned long long& checksum) {
    bool wrong = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const T got = __hip_atomic_load(p[j], __ATOMIC_RELAXED, SCOPE);
      wrong |= got != (T)expected[j * 64 + lane];
      checksum ^= (unsigned long long)got << (sizeof(T) == 4 ? 32 * (j & 1) : 0);
    }
    return wrong;
  }
};

// the u64 LDS cell: add, xor
struct AtomicLds64Lane {
  typedef AtomicInt<unsigned long long, __HIP_MEMORY_SCOPE_WORKGROUP> A;
  unsigned long long* p[1];
  unsigned long long m[1];
  __device__ __forceinline__ void seed(unsigned sd, int sec, int lane) {
    m[0] = valu_seed_state(sd, sec, 4 * 64 + lane);
    __hip_atomic_store(p[0], m[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ void step(unsigned c, AtomicLaneCheck& chk, int op_base) {
    unsigned long long x, old;
    HVD_ATOMIC_PAIR(0, 0, add, m[0] + x)
    HVD_ATOMIC_PAIR(1, 0, xor_, m[0] ^ x)
  }
};
#undef HVD_ATOMIC_PAIR

__device__ __forceinline__ unsigned f16_bits(int v) {
  return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)v);
}
__device__ __forceinline__ unsigned bf16_bits(int v) {  // exact for |v| <= 256
  return __float_as_uint((float)v) >> 16;
}
__device__ __forceinline__ unsigned long long f64_bits(long long v) {
  return (unsigned long long)__double_as_longlong((double)v);
}

// The float cells of one lane: byte offsets in the wave's region f64 add 0,
// f64 min/max 512, f32 1024, packed f16 1280, packed bf16 1536. The mirrors
// are integers: the sums are exact while ops.atomic_fp_exact holds.
template <bool LDS, int SCOPE> struct AtomicFpLane {
  float* pf;
  double* pd;
  double* pm;
  unsigned* ph;
  unsigned* pb;
  int f, h0, h1, b0, b1;
  long long d, mm;
  __device__ __forceinline__ void init(unsigned char* wave_base, int lane) {
    pd = reinterpret_cast<double*>(wave_base) + lane;
    pm = reinterpret_cast<double*>(wave_base + 512) + lane;
    pf = reinterpret_cast<float*>(wave_base + 1024) + lane;
    ph = reinterpret_cast<unsigned*>(wave_base + 1280) + lane;
    pb = reinterpret_cast<unsigned*>(wave_base + 1536) + lane;
  }
  static __device__ __forceinline__ unsigned pk_f16(unsigned* p, unsigned bits) {
    const f16x2 v = __builtin_bit_cast(f16x2, bits);
    if constexpr (LDS)
      return __builtin_bit_cast(unsigned, __builtin_amdgcn_ds_atomic_fadd_v2f16(
          (__attribute__((address_space(3))) f16x2*)p, v));
    else
      return __builtin_bit_cast(unsigned, __builtin_amdgcn_global_atomic_fadd_v2f16(
          (__attribute__((address_space(1))) f16x2*)p, v));
  }
  static __device__ __forceinline__ unsigned pk_bf16(unsigned* p, unsigned bits) {
    const bf16x2 v = __builtin_bit_cast(bf16x2, bits);
    if constexpr (LDS)
      return __builtin_bit_cast(unsigned, __builtin_amdgcn_ds_atomic_fadd_v2bf16(
          (__attribute__((address_space(3))) bf16x2*)p, v));
    else
      return __builtin_bit_cast(unsigned, __builtin_amdgcn_global_atomic_fadd_v2bf16(
          (__attribute__((address_space(1))) bf16x2*)p, v));
  }
  // j0: the index of the f32 cell among the section's cells
  __device__ __forceinline__ void seed(unsigned sd, int sec, int lane, int j0) {
    const unsigned long long sf = valu_seed_state(sd, sec, j0 * 64 + lane);
    const unsigned long long sdd = valu_seed_state(sd, sec, (j0 + 1) * 64 + lane);
    const unsigned long long sm = valu_seed_state(sd, sec, (j0 + 2) * 64 + lane);
    const unsigned sh = (unsigned)valu_seed_state(sd, sec, (j0 + 3) * 64 + lane);
    const unsigned sb = (unsigned)valu_seed_state(sd, sec, (j0 + 4) * 64 + lane);
    f = (int)((unsigned)sf & 0xFFFFFu) - 0x80000;
    d = (long long)(sdd & ((1ull << 50) - 1)) - (1ll << 49);
    mm = (long long)(sm & ((1ull << 50) - 1)) - (1ll << 49);
    h0 = (int)(sh & 511u) - 256;
    h1 = (int)((sh >> 16) & 511u) - 256;
    b0 = (int)(sb & 63u) - 32;
    b1 = (int)((sb >> 16) & 63u) - 32;
    __hip_atomic_store(pf, (float)f, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_store(pd, (double)d, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_store(pm, (double)mm, __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_store(ph, f16_bits(h0) | (f16_bits(h1) << 16), __ATOMIC_RELAXED, SCOPE);
    __hip_atomic_store(pb, bf16_bits(b0) | (bf16_bits(b1) << 16), __ATOMIC_RELAXED, SCOPE);
  }
  __device__ __forceinline__ void inject(int bit) {
    (void)__hip_atomic_fetch_xor(reinterpret_cast<unsigned*>(pf), 1u << bit, __ATOMIC_RELAXED,
                                 SCOPE);
  }
  __device__ __forceinline__ void step(unsigned c, AtomicLaneCheck& chk, int op_base) {
#pragma unroll
    for (int form = 0; form < 2; form++) {  // add f32
      const int x = (int)(atomic_operand((unsigned)f, c, form) % 2047u) - 1023;
      const float old = __hip_atomic_fetch_add(pf, (float)x, __ATOMIC_RELAXED, SCOPE);
      if (form == 0) chk.see(__float_as_uint(old) != __float_as_uint((float)f), op_base);
      f += x;
    }
#pragma unroll
    for (int form = 0; form < 2; form++) {  // add f64
      const long long x =
          (long long)(atomic_operand((unsigned long long)d, c, 2 + form) & ((1ull << 41) - 1)) -
          (1ll << 40);
      const double old = __hip_atomic_fetch_add(pd, (double)x, __ATOMIC_RELAXED, SCOPE);
      if (form == 0)
        chk.see((unsigned long long)__double_as_longlong(old) != f64_bits(d), op_base + 2);
      d += x;
    }
#pragma unroll
    for (int form = 0; form < 4; form++) {  // min f64 (forms 0, 1), max f64 (forms 2, 3)
      const long long x =
          (long long)(atomic_operand((unsigned long long)mm, c, 4 + form) & ((1ull << 52) - 1)) -
          (1ll << 51);
      const double old = form < 2 ? __hip_atomic_fetch_min(pm, (double)x, __ATOMIC_RELAXED, SCOPE)
                                  : __hip_atomic_fetch_max(pm, (double)x, __ATOMIC_RELAXED, SCOPE);
      if ((form & 1) == 0)
        chk.see((unsigned long long)__double_as_longlong(old) != f64_bits(mm), op_base + 4 + form);
      mm = form < 2 ? (x < mm ? x : mm) : (x > mm ? x : mm);
    }
#pragma unroll
    for (int form = 0; form < 2; form++) {  // pk_add f16
      const unsigned mirror = f16_bits(h0) | (f16_bits(h1) << 16);
      const unsigned h = atomic_operand(mirror, c, 8 + form);
      const int x0 = (int)((h & 0xFFFFu) % 31u) - 15, x1 = (int)((h >> 16) % 31u) - 15;
      const unsigned old = pk_f16(ph, f16_bits(x0) | (f16_bits(x1) << 16));
      if (form == 0) chk.see(old != mirror, op_base + 8);
      h0 += x0;
      h1 += x1;
    }
#pragma unroll
    for (int form = 0; form < 2; form++) {  // pk_add bf16
      const unsigned mirror = bf16_bits(b0) | (bf16_bits(b1) << 16);
      const unsigned h = atomic_operand(mirror, c, 10 + form);
      const int x0 = (int)((h & 0xFFFFu) % 7u) - 3, x1 = (int)((h >> 16) % 7u) - 3;
      const unsigned old = pk_bf16(pb, bf16_bits(x0) | (bf16_bits(x1) << 16));
      if (form == 0) chk.see(old != mirror, op_base + 10);
      b0 += x0;
      b1 += x1;
    }
  }
  // expected: the f32 cell, lane 0
  __device__ __forceinline__ bool wrong_final(const long long* expected, int lane,
                                              unsigned long long& checksum) {
    const unsigned gf =
        __hip_atomic_load(reinterpret_cast<unsigned*>(pf), __ATOMIC_RELAXED, SCOPE);
    const unsigned long long gd =
        __hip_atomic_load(reinterpret_cast<unsigned long long*>(pd), __ATOMIC_RELAXED, SCOPE);
    const unsigned long long gm =
        __hip_atomic_load(reinterpret_cast<unsigned long long*>(pm), __ATOMIC_RELAXED, SCOPE);
    const unsigned gh = __hip_atomic_load(ph, __ATOMIC_RELAXED, SCOPE);
    const unsigned gb = __hip_atomic_load(pb, __ATOMIC_RELAXED, SCOPE);
    checksum ^= gd ^ gm ^ ((unsigned long long)gf << 32) ^ gh ^ ((unsigned long long)gb << 32);
    return gf != (unsigned)expected[lane] || gd != (unsigned long long)expected[64 + lane] ||
           gm != (unsigned long long)expected[128 + lane] ||
           gh != (unsigned)expected[192 + lane] || gb != (unsigned)expected[256 + lane];
  }
};

template <int SEC>
__global__ void __launch_bounds__(256)
atomic_burn_kernel(const long long* __restrict__ expected, unsigned char* __restrict__ cells,
                   long wave_bytes, int4* __restrict__ records, unsigned seed, int chain,
                   int rounds, int inject_wave, int inject_round, int inject_lane,
                   int inject_bit) {
  constexpr bool kLds = SEC == ATOMIC_LDS;
  constexpr bool kInt = SEC != ATOMIC_GFP;
  constexpr bool kFp = SEC == ATOMIC_GFP || kLds;
  constexpr int kScope = kLds ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  constexpr int kFinalOp = kLds ? ATOMIC_INT_OPS + ATOMIC_U64_OPS + ATOMIC_FP_OPS
                           : kInt ? ATOMIC_INT_OPS : ATOMIC_FP_OPS;
  typedef typename std::conditional<SEC == ATOMIC_G64, unsigned long long, unsigned>::type T;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLds ? 4 * ATOMIC_LDS_WAVE_BYTES : 16];
  __shared__ unsigned short owner[kLds ? 256 * ATOMIC_LDS_MAX_CHAIN : 2];
  __shared__ unsigned ticket_word[2];
  const int lane = threadIdx.x & 63;
  const int wave = uniform_wave_index();
  const unsigned place = hw_word();

  // an LDS wave region: the u64 cell at 0, the u32 cells at 512, the float cells at 1536
  unsigned char* base = kLds ? lds + (threadIdx.x >> 6) * ATOMIC_LDS_WAVE_BYTES
                             : cells + (long)wave * wave_bytes;
  AtomicIntLane<T, kScope> ints;
  AtomicLds64Lane wide;
  AtomicFpLane<kLds, kScope> fp;
  if constexpr (kInt) ints.init(base + (kLds ? 512 : 0), lane);
  if constexpr (kLds) wide.p[0] = reinterpret_cast<unsigned long long*>(base) + lane;
  if constexpr (kFp) fp.init(base + (kLds ? 1536 : 0), lane);

  const bool inject_here = wave == inject_wave && lane == inject_lane;
  int mismatched = 0, first_round = -1, first_lane = -1, first_op = -1;
  unsigned long long checksum = 0;
  for (int round = 0; round < rounds; round++) {
    if constexpr (kInt) ints.seed(seed, SEC, lane);
    if constexpr (kLds) wide.seed(seed, SEC, lane);
    if constexpr (kFp) fp.seed(seed, SEC, lane, kLds ? 5 : 0);
    if (inject_here && round == inject_round) {
      if constexpr (kInt) ints.inject(inject_bit);
      else fp.inject(inject_bit);
    }
    AtomicLaneCheck chk;
    unsigned bad_steps = 0;
    for (int c = 0; c < chain; c++) {
      chk.bad = 0;
      if constexpr (kInt) ints.step((unsigned)c, chk, 0);
      if constexpr (kLds) wide.step((unsigned)c, chk, ATOMIC_INT_OPS);
      if constexpr (kFp) fp.step((unsigned)c, chk, kLds ? ATOMIC_INT_OPS + ATOMIC_U64_OPS : 0);
      bad_steps += chk.bad;
    }
    bool wrong = false;
    if constexpr (kInt) wrong |= ints.wrong_final(expected, lane, checksum);
    if constexpr (kLds) {
      const unsigned long long got =
          __hip_atomic_load(wide.p[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      wrong |= got != (unsigned long long)expected[4 * 64 + lane];
      checksum ^= got;
    }
    if constexpr (kFp) wrong |= fp.wrong_final(expected + (kLds ? 5 * 64 : 0), lane, checksum);
    if (wrong) {
      bad_steps++;
      if (chk.first_op < 0) chk.first_op = kFinalOp;
    }
    const unsigned total = wave_add(bad_steps);
    mismatched += (int)total;
    if (total != 0 && first_round < 0) {
      first_round = round;
      first_lane = (int)wave_min(bad_steps ? (unsigned)lane : 64u);
      first_op = (int)wave_min(lane == first_lane ? (unsigned)chk.first_op : 0x7FFFFFFFu);
    }
  }
  checksum = wave_xor(checksum);

  unsigned ticket_faults = 0;
  if constexpr (kLds) {
    const unsigned draws = 256u * (unsigned)chain;  // chain <= ATOMIC_LDS_MAX_CHAIN (host check)
    for (unsigned i = threadIdx.x; i < draws; i += 256) owner[i] = 0;
    if (threadIdx.x == 0) ticket_word[0] = 0;
    __syncthreads();
    // an index the compiler cannot prove uniform: every lane issues its own
    // ds_add_rtn_u32 (a uniform address is rewritten into one add per wave)
    int zero = 0;
    asm volatile("" : "+v"(zero));
    unsigned out_of_range = 0;
    for (int c = 0; c < chain; c++) {
      const unsigned t = __hip_atomic_fetch_add(&ticket_word[zero], 1u, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
      if (t < draws) owner[t] = (unsigned short)(threadIdx.x + 1);
      else out_of_range++;
    }
    __syncthreads();
    unsigned holes = 0;
    for (unsigned i = lane; i < draws; i += 64) holes += owner[i] == 0;
    ticket_faults = wave_add(holes + out_of_range) + (ticket_word[0] != draws);
  }
  if (lane == 0)
    store_record8(records, wave, (int)place, mismatched, first_round, first_lane,
                  (int)(unsigned)checksum, (int)(unsigned)(checksum >> 32), first_op,
                  (int)ticket_faults);
}

static int atomic_section_id(const std::string& section) {
  return section == "g32" ? ATOMIC_G32 : section == "g64" ? ATOMIC_G64
         : section == "gfp" ? ATOMIC_GFP : section == "lds" ? ATOMIC_LDS : -1;
}

// expected: int64 on the current device, cell j of lane l at [j*64 + l], the
// raw bits of the final cell values (ops.atomic_burn_expected): 4 cells for
// g32 and g64, 5 for gfp, 10 for lds. One untimed warm-up launch, then one
// timed launch (warm_then_timed_ms); each launch seeds its own cells.
// Returns (records [waves,8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> atomic_burn(torch::Tensor expected, const std::string& section,
                                              long seed, long blocks, long chain, long rounds,
                                              long inject_wave, long inject_round,
                                              long inject_lane, long inject_bit) {
  const int sec = atomic_section_id(section);
  TORCH_CHECK(sec >= 0, "section must be one of g32, g64, gfp, lds; got ", section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 14), "blocks must be in [1, 2^14]");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  // bounded run (BENCHMARKS.md "Atomic probe"): a step of the slowest section,
  // g64, measures ~118 us at 2048 workgroups and ~960 us at 16384 (the time
  // grows with the grid: ~58 ns per workgroup-step); 2^22 workgroup-steps
  // are ~0.24 s, a quarter of a second. A grid too small to be bound by
  // throughput is bound by the step's latency instead: see the 2^12-step cap's
  // arithmetic in BENCHMARKS.md
  TORCH_CHECK(chain <= (1L << 12) && rounds <= (1L << 12) && chain * rounds <= (1L << 12),
              "chain*rounds must be <= 2^12");
  TORCH_CHECK(blocks * chain * rounds <= (1L << 22), "blocks*chain*rounds must be <= 2^22");
  TORCH_CHECK(sec != ATOMIC_LDS || chain <= ATOMIC_LDS_MAX_CHAIN,
              "section lds: chain must be <= ", (int)ATOMIC_LDS_MAX_CHAIN,
              " (the ticket's owner table lives in LDS)");
  const long bits = sec == ATOMIC_G64 ? 64 : 32;
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds && inject_lane >= -1 && inject_lane < 64 &&
                  inject_bit >= -1 && inject_bit < bits,
              "inject_wave/inject_round/inject_lane/inject_bit out of range");
  TORCH_CHECK(inject_wave < 0 || (inject_round >= 0 && inject_lane >= 0 && inject_bit >= 0),
              "an injection needs inject_round, inject_lane and inject_bit");
  const long ncells = sec == ATOMIC_GFP ? 5 : sec == ATOMIC_LDS ? 10 : 4;
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  TORCH_CHECK(expected.is_cuda() && expected.get_device() == dev,
              "expected must be on the current GPU");
  TORCH_CHECK(expected.dtype() == torch::kInt64 && expected.numel() == ncells * 64,
              "expected must hold ", ncells * 64, " int64 values for section ", section);
  expected = expected.contiguous();
  const long long* want = reinterpret_cast<const long long*>(expected.data_ptr<int64_t>());
  const long wave_bytes = sec == ATOMIC_G32 ? 1024 : sec == ATOMIC_G64 ? 2048
                          : sec == ATOMIC_GFP ? (long)ATOMIC_FP_BYTES : 0;
  auto cells = torch::zeros({std::max(blocks * 4 * wave_bytes, 256L)},
                            torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA));
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<4>(sec, [&](auto sec_c) {
      hipLaunchKernelGGL(atomic_burn_kernel<decltype(sec_c)::value>, dim3(blocks), dim3(256), 0,
                         stream, want, cells.data_ptr<uint8_t>(), wave_bytes,
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (unsigned)seed,
                         (int)chain, (int)rounds, (int)inject_wave, (int)inject_round,
                         (int)inject_lane, (int)inject_bit);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// Atomic probe, part 2: contention on shared cells (ops.atomic_contend).
//
// `cells` shared cells sit 4 KiB apart (512 int64 each); lane gid of a
// 256-lane workgroup works on cell gid % cells, so the lanes on a cell come
// from every workgroup, hence from every CU and XCD the grid reaches. The
// host zeroes or seeds every buffer before the launch and computes every
// verdict from the buffers copied back after it: the kernel boundary is the
// only synchronisation, and no wave waits for another.
//   ticket: `per_lane` returning agent-scope fetch_add(1) on the cell's
//           counter; owner[cell][ticket] = gid + 1 by a plain store,
//           range-checked against the draws on that cell; a lane also checks
//           that its own tickets increase.
//   reduce: thirteen non-returning forms, one 128-byte slot of the cell each
//           (slot k at int64 index 16*k): add u32, add u64, xor, or, and, umin,
//           umax, smin, smax, add f32, add f64, pk_add bf16, pk_add f16. The
//           float contributions are integers whose every partial sum is exact,
//           so the result does not depend on the arrival order.
//   cas:    `per_lane` adds of the lane's value by a cmpswap loop. A failed
//           cmpswap means another lane's succeeded; N = lanes on the cell *
//           per_lane succeed in the whole launch, so a lane can fail at most
//           N - 1 times: a lane that fails N times gives up, which is a fault.
// Record per wave: {hw word, non-increasing tickets, out-of-range tickets,
// lanes that gave up, failed cmpswaps, 0, 0, 0}.
// ---------------------------------------------------------------------------
enum { CONTEND_TICKET = 0, CONTEND_REDUCE = 1, CONTEND_CAS = 2 };
enum { CONTEND_CELL_WORDS = 512 };  // int64 per cell: 4 KiB

__device__ __forceinline__ int contend_lanes_on_cell(int lanes, int cells, int cell) {
  return lanes / cells + (cell < lanes % cells);
}

__global__ void __launch_bounds__(256)
atomic_ticket_kernel(unsigned long long* __restrict__ shared, int* __restrict__ owner,
                     int4* __restrict__ records, int per_lane, int cells, int width) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int lanes = gridDim.x * 256;
  const int cell = gid % cells;
  const unsigned draws = (unsigned)(contend_lanes_on_cell(lanes, cells, cell) * per_lane);
  unsigned* counter = reinterpret_cast<unsigned*>(shared + (long)cell * CONTEND_CELL_WORDS);
  unsigned previous = 0, not_increasing = 0, out_of_range = 0;
  for (int j = 0; j < per_lane; j++) {
    const unsigned t =
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t < draws) owner[(long)cell * width + t] = gid + 1;  // draws <= width (host)
    else out_of_range++;
    if (j > 0 && t <= previous) not_increasing++;
    previous = t;
  }
  const unsigned place = hw_word();
  not_increasing = wave_add(not_increasing);
  out_of_range = wave_add(out_of_range);
  if ((threadIdx.x & 63) == 0)
    store_record8(records, gid >> 6, (int)place, (int)not_increasing, (int)out_of_range, 0, 0, 0,
                  0, 0);
}

__global__ void __launch_bounds__(256)
atomic_reduce_kernel(unsigned long long* __restrict__ shared, int4* __restrict__ records,
                     unsigned seed, int per_lane, int cells) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int cell = gid % cells;
  unsigned long long* slot = shared + (long)cell * CONTEND_CELL_WORDS;
  typedef __attribute__((address_space(1))) bf16x2* gbf;
  typedef __attribute__((address_space(1))) f16x2* gf16;
#define SLOT(K, TYPE) reinterpret_cast<TYPE*>(slot + 16 * (K))
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
  for (int j = 0; j < per_lane; j++) {
    const unsigned n = (unsigned)(gid / cells) * (unsigned)per_lane + (unsigned)j;
    const unsigned h = fmix32(seed + (unsigned)gid * 0x9E3779B1u + (unsigned)j * 0x85EBCA6Bu);
    unsigned hk[13];
#pragma unroll
    for (int k = 0; k < 13; k++) hk[k] = fmix32(h + (unsigned)k * 0x632BE5ABu);
    (void)__hip_atomic_fetch_add(SLOT(0, unsigned), hk[0], RLX_AGENT);
    (void)__hip_atomic_fetch_add(SLOT(1, unsigned long long),
                                 ((unsigned long long)hk[1] << 32) | h, RLX_AGENT);
    (void)__hip_atomic_fetch_xor(SLOT(2, unsigned), hk[2], RLX_AGENT);
    (void)__hip_atomic_fetch_or(SLOT(3, unsigned), n < 24u ? 1u << (hk[3] & 31) : 0u, RLX_AGENT);
    (void)__hip_atomic_fetch_and(SLOT(4, unsigned), n < 24u ? ~(1u << (hk[4] & 31)) : ~0u,
                                 RLX_AGENT);
    (void)__hip_atomic_fetch_min(SLOT(5, unsigned), hk[5], RLX_AGENT);
    (void)__hip_atomic_fetch_max(SLOT(6, unsigned), hk[6], RLX_AGENT);
    (void)__hip_atomic_fetch_min(SLOT(7, int), (int)hk[7], RLX_AGENT);
    (void)__hip_atomic_fetch_max(SLOT(8, int), (int)hk[8], RLX_AGENT);
    (void)__hip_atomic_fetch_add(SLOT(9, float), (float)((int)(hk[9] % 257u) - 128), RLX_AGENT);
    (void)__hip_atomic_fetch_add(SLOT(10, double), (double)(int)hk[10], RLX_AGENT);
    const bool active = n < 128u;
    const unsigned b = active ? bf16_bits(hk[11] & 1 ? 1 : -1) | (bf16_bits(hk[11] & 2 ? 1 : -1) << 16)
                              : 0u;
    (void)__builtin_amdgcn_global_atomic_fadd_v2bf16((gbf)SLOT(11, unsigned),
                                                     __builtin_bit_cast(bf16x2, b));
    const unsigned f = active ? f16_bits((int)((hk[12] & 0xFFFFu) % 33u) - 16) |
                                    (f16_bits((int)((hk[12] >> 16) % 33u) - 16) << 16)
                              : 0u;
    (void)__builtin_amdgcn_global_atomic_fadd_v2f16((gf16)SLOT(12, unsigned),
                                                    __builtin_bit_cast(f16x2, f));
  }
#undef SLOT
#undef RLX_AGENT
  const unsigned place = hw_word();
  if ((threadIdx.x & 63) == 0)
    store_record8(records, gid >> 6, (int)place, 0, 0, 0, 0, 0, 0, 0);
}

__global__ void __launch_bounds__(256)
atomic_cas_kernel(unsigned long long* __restrict__ shared, int4* __restrict__ records,
                  unsigned seed, int per_lane, int cells) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int lanes = gridDim.x * 256;
  const int cell = gid % cells;
  const int cap = contend_lanes_on_cell(lanes, cells, cell) * per_lane;
  unsigned long long* p = shared + (long)cell * CONTEND_CELL_WORDS;
  const unsigned long long v = mix64(((unsigned long long)seed << 32) | (unsigned)gid);
  unsigned long long current =
      __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int done = 0, failed = 0;
  for (int tries = 0; tries < per_lane + cap; tries++) {
    if (done >= per_lane || failed >= cap) break;
    unsigned long long seen = current;
    if (__hip_atomic_compare_exchange_strong(p, &seen, current + v, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
      done++;
      current += v;
    } else {
      failed++;
      current = seen;
    }
  }
  const unsigned place = hw_word();
  const unsigned gave_up = wave_add((unsigned)(done < per_lane));
  const unsigned retries = wave_add((unsigned)failed);
  if ((threadIdx.x & 63) == 0)
    store_record8(records, gid >> 6, (int)place, 0, 0, (int)gave_up, (int)retries, 0, 0, 0);
}

// Returns {"shared": int64 [cells, 512] (the cells after the launch; ticket:
// the counter is the low word of [c, 0]; reduce: slot k at [c, 16*k]; cas: the
// sum at [c, 0]), "owner": int32 [cells, width] (ticket; else [cells, 0]),
// "records": int32 [blocks*4, 8], "ms": the launch between two events}. One
// launch on throw-away buffers first, so that the timed one is warm.
py::dict atomic_contend(const std::string& section, long seed, long blocks, long per_lane,
                        long cells) {
  const int sec = section == "ticket" ? CONTEND_TICKET : section == "reduce" ? CONTEND_REDUCE
                  : section == "cas" ? CONTEND_CAS : -1;
  TORCH_CHECK(sec >= 0, "section must be one of ticket, reduce, cas; got ", section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 13), "blocks must be in [1, 2^13]");
  TORCH_CHECK(per_lane >= 1 && per_lane <= 64, "per_lane must be in [1, 64]");
  const long lanes = blocks * 256;
  TORCH_CHECK(cells >= 1 && cells <= 4096 && cells <= lanes,
              "cells must be in [1, min(4096, blocks*256)]");
  // bounded run and exact floats (BENCHMARKS.md "Atomic probe"): at most 2^16
  // operations on one cell (f32: 2^16 contributions of at most 128 stay below
  // 2^24) and 2^23 in the launch: milliseconds. The cmpswap loop is bounded by
  // its attempts: a success fails at most the other lanes of its cell once, so
  // a cell sees at most lanes-on-it x successes-on-it of them, and one word
  // takes ~88 atomics/us, all cells together ~5500: at most 2^14 successes and
  // 2^26 attempts on a cell (measured there: 2^23.9 attempts, 179 ms) and 2^30
  // over all cells (measured there, 256 cells: 8 ms)
  const long lanes_on_cell = (lanes + cells - 1) / cells;
  const long on_cell = lanes_on_cell * per_lane;
  const long cap_cell = sec == CONTEND_CAS ? (1L << 14) : (1L << 16);
  TORCH_CHECK(on_cell <= cap_cell, "at most ", cap_cell, " operations on one cell; got ", on_cell);
  if (sec == CONTEND_CAS) {
    TORCH_CHECK(lanes_on_cell * on_cell <= (1L << 26) &&
                    cells * lanes_on_cell * on_cell <= (1L << 30),
                "cas: lanes on a cell x operations on it must be <= 2^26, and <= 2^30 summed "
                "over the cells");
  } else {
    TORCH_CHECK(lanes * per_lane <= (1L << 23), "at most 2^23 operations; got ",
                lanes * per_lane);
  }
  const long width = sec == CONTEND_TICKET ? on_cell : 0;
  auto init = torch::zeros({cells, (long)CONTEND_CELL_WORDS}, torch::kInt64);
  int64_t* w = init.data_ptr<int64_t>();
  for (long c = 0; c < cells; c++) {
    int64_t* cell = w + c * CONTEND_CELL_WORDS;
    if (sec == CONTEND_REDUCE) {
      cell[16 * 4] = 0xFFFFFFFFLL;  // and
      cell[16 * 5] = 0xFFFFFFFFLL;  // umin
      cell[16 * 7] = 0x7FFFFFFFLL;  // smin
      cell[16 * 8] = 0x80000000LL;  // smax
    } else if (sec == CONTEND_CAS) {
      unsigned long long x = ((unsigned long long)(unsigned)seed << 32) ^ (unsigned long long)c;
      x += 0x9E3779B97F4A7C15ull;  // splitmix64, as mix64 on the device
      x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
      x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
      cell[0] = (int64_t)(x ^ (x >> 31));
    }
  }
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](torch::Tensor& shared, torch::Tensor& owner, torch::Tensor& records) {
    unsigned long long* sp = reinterpret_cast<unsigned long long*>(shared.data_ptr<int64_t>());
    int4* rp = reinterpret_cast<int4*>(records.data_ptr<int>());
    if (sec == CONTEND_TICKET)
      hipLaunchKernelGGL(atomic_ticket_kernel, dim3(blocks), dim3(256), 0, stream, sp,
                         owner.data_ptr<int>(), rp, (int)per_lane, (int)cells, (int)width);
    else if (sec == CONTEND_REDUCE)
      hipLaunchKernelGGL(atomic_reduce_kernel, dim3(blocks), dim3(256), 0, stream, sp, rp,
                         (unsigned)seed, (int)per_lane, (int)cells);
    else
      hipLaunchKernelGGL(atomic_cas_kernel, dim3(blocks), dim3(256), 0, stream, sp, rp,
                         (unsigned)seed, (int)per_lane, (int)cells);
  };
  torch::Tensor shared, owner, records;
  double ms = 0;
  for (int timed = 0; timed < 2; timed++) {
    shared = init.to(torch::kCUDA);
    owner = torch::zeros({cells, width},
                         torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA));
    records = zero_records(blocks * 4, 8);
    ms = timed_ms(stream, [&]() { launch(shared, owner, records); });
  }
  py::dict d;
  d["shared"] = shared;
  d["owner"] = owner;
  d["records"] = records;
  d["ms"] = ms;
  return d;
}

// ---------------------------------------------------------------------------
// Memory-path probe: how production GEMM and attention kernels move tiles,
// which no kernel above executes. Four sections, one kernel each (SEC):
//   buf    raw buffer loads and stores in every width, the byte address split
//          between voffset, soffset and the immediate differently per step,
//          cross-checked against plain global stores and loads
//   oob    the descriptor's hardware bounds check at sharp lengths: an access
//          wholly in range returns the data, one wholly out returns 0 and its
//          store is dropped
//   lds    direct-to-LDS loads (global_load_lds_dword/x4, buffer_load_dword/x4
//          ... lds), read back with ds_read_b128
//   forms  the sub-dword, d16 and wide forms on the global and the LDS path
//          that the marches leave out
// All of it is data movement, so every result is exact and the host mirror
// (ops/mempath_probe.py) states it bit for bit.
//
// Memory: one int32 row of MP_ROW_WORDS per wave, a slice of 3072 words the
// wave fills and moves around and behind it a guard of 64 words whose every
// byte is non-zero (MP_GUARD_SENTINEL). A wave only reads what it wrote
// itself, after an agent-scope fence; no wave waits for another and every loop
// bound is a launch argument. The value of word i in round r is
//   v(i) = fmix32((seed + r*0x9E3779B9 + wave*0x7F4A7C15) ^ (i*0x85EBCA6B)),
// complemented in odd rounds: a bijection in i, so an address alias reads back
// as wrong data, and every bit travels each path holding 0 and holding 1.
//
// A section is a fixed list of steps (ops.mempath_steps names them); the
// global step index is round*n_steps + step. Store steps write v ^ (step+1)*
// 0x9E3779B9 and are read back through another form.
//
// Safety of the oob section: every address an instruction would form without
// the check, base + voffset + soffset + imm + width, lies inside the wave's own
// row (static_asserts below, asserted again per case by ops.mempath_oob_cases),
// soffset is 0, and an access that straddles the length is never issued. A
// wrong descriptor or a broken check reads a sentinel or dirties the guard,
// which the step itself and the round's last step (the guard read with plain
// loads) report; it cannot fault. Word 3 of the descriptor, 0x00020000, is
// what Composable Kernel uses for raw buffers on the gfx9 family
// (CK_BUFFER_RESOURCE_3RD_DWORD in ck/ck.hpp of the ROCm installation).
//
// Layout of a direct-to-LDS load, from the LLVM AMDGPU description of
// llvm.amdgcn.global.load.lds / raw.ptr.buffer.load.lds (the LDS base goes to
// M0, the immediate offset applies to the memory and the LDS address) and
// ck_tile's async_buffer_load_dwordxn_v / amd_direct_load_global_to_lds: lane
// l's N bytes land at M0 base + imm + l*N. The host mirror is written from
// that, not from what the kernel returns. What an out-of-range lane of
// `buffer_load_dword ... lds` does to LDS (writes 0 or leaves it) is recorded
// in field [7] (1 = zero, 2 = left alone), not judged.
//
// Per wave, lane 0 writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word)
//   [1] mismatched elements
//   [2] first bad global step (-1 if none)
//   [3] lowest bad byte offset within that step (-1 if none)
//   [4] dropped mask, [5] raised mask, of the compared element zero-extended
//   [6] sum mod 2^32 of every value compared in the even rounds
//   [7] flags (lds section, see above; forms: the other half after a d16
//       load, 1 kept, 2 zeroed, 4 neither), else 0
//
// inject_* (default -1 = off): in wave 0 of block inject_block, at global step
// inject_step, lane 0 flips bit inject_bit of the element at byte offset
// inject_offset of what the step is about to read: the slice (flipped back
// after a load step, so later steps see clean data), the read-back target of a
// store step after the store, the LDS region after a direct load. A plain
// store into the wave's own memory. In the oob section injection instead
// lengthens the descriptor of all four waves of the block so that the first
// wholly-out access of that step is in range: it returns (or overwrites, and
// the step restores) slice or guard data inside the row.
//
// Checked in the gfx950 disassembly: each step issues the form it is named
// after, with one exception: of the four signed sub-dword loads of a batch
// that the builtins and plain C++ produce (buffer_load_sbyte/sshort,
// global_load_sbyte/sshort, ds_read_i8/i16) the compiler emits one as the
// unsigned load and a v_bfe_i32, so both appear in those steps. The compiler
// merges neighbouring accesses and splits wide ones; the empty asm with a
// memory clobber after an access keeps it single, as in the LDS march, and
// the d16, wide LDS and read2/write2 forms are inline asm. The new code has
// no floating-point arithmetic. gfx950 build: buf 121, oob 44, lds 62 and
// forms 70 VGPRs, no scratch; lds and forms hold 64 KiB of LDS, so
// two of their workgroups fit a CU.
// ---------------------------------------------------------------------------
constexpr int MP_SLICE_WORDS = 3072;  // 64 lanes x 12 B and 64 x 16 B divide it
constexpr int MP_GUARD_WORDS = 64;
constexpr int MP_ROW_WORDS = MP_SLICE_WORDS + MP_GUARD_WORDS;
constexpr int MP_SLICE_BYTES = 4 * MP_SLICE_WORDS;
constexpr int MP_ROW_BYTES = 4 * MP_ROW_WORDS;
constexpr int MP_LDS_WAVE_WORDS = 4096;  // 16 KiB of the 64 KiB per wave
constexpr unsigned MP_GUARD_SENTINEL = 0xC3A5E17Bu;  // every byte non-zero
constexpr unsigned MP_LDS_SENTINEL = 0x5AA5C33Cu;
constexpr unsigned MP_OOB_MARKER = 0xD1B2E4F7u;
constexpr unsigned MP_D16_CANARY = 0x9C6A3B57u;  // preset in a d16 load's register
constexpr int MP_RSRC_WORD3 = 0x00020000;
enum { MP_BUF = 0, MP_OOB, MP_LDS, MP_FORMS, MP_SECTIONS };
constexpr int MP_STEPS[MP_SECTIONS] = {14, 61, 5, 39};
// oob: lanes 0..15 access offsets lo + lane*W in a window across the length L
__host__ __device__ constexpr int mp_oob_length(int li) {
  return li == 0 ? MP_SLICE_BYTES : li == 1 ? MP_SLICE_BYTES - 1 : li == 2 ? MP_SLICE_BYTES - 3
                                                                 : li == 3 ? 4 : 0;
}
constexpr int MP_OOB_LANES = 16;
constexpr int MP_OOB_MAX_WIDTH = 16;
__host__ __device__ constexpr int mp_oob_lo(int L, int W) {
  return L / W * W - (MP_OOB_LANES / 2) * W < 0 ? 0 : L / W * W - (MP_OOB_LANES / 2) * W;
}
__host__ __device__ constexpr int mp_oob_first_out(int L, int W) { return (L + W - 1) / W * W; }
static_assert(mp_oob_lo(MP_SLICE_BYTES, MP_OOB_MAX_WIDTH) + MP_OOB_LANES * MP_OOB_MAX_WIDTH <=
                      MP_ROW_BYTES &&
                  mp_oob_lo(MP_SLICE_BYTES, 12) + MP_OOB_LANES * 12 <= MP_ROW_BYTES,
              "every oob window must end inside the row");
static_assert(MP_ROW_BYTES % 16 == 0 && MP_SLICE_BYTES % (64 * 12) == 0 &&
                  MP_SLICE_BYTES % (4 * 64 * 16) == 0,
              "rows stay 16 B aligned and every width tiles the slice in batches of four");
// lds: where in the wave's 16 KiB each step's copy of the slice starts (bytes)
__host__ __device__ constexpr int mp_lds_dst(int step) {
  constexpr int dst[5] = {0, 4096, 2048, 16, 512};
  return dst[step];
}
constexpr int MP_LDS_OOB_INRANGE = 32;  // lanes of the last step the descriptor covers

typedef unsigned mp_u2 __attribute__((ext_vector_type(2)));
typedef unsigned mp_u3 __attribute__((ext_vector_type(3)));
typedef unsigned mp_u4 __attribute__((ext_vector_type(4)));
#define MP_LDS_AS __attribute__((address_space(3)))

struct MpPat {
  unsigned rs, inv;
  __device__ __forceinline__ unsigned word(int i) const {
    return fmix32(rs ^ ((unsigned)i * 0x85EBCA6Bu)) ^ inv;
  }
  // the row as it must stand: the slice, then the guard
  __device__ __forceinline__ unsigned row_word(int i) const {
    return i < MP_SLICE_WORDS ? word(i) : MP_GUARD_SENTINEL;
  }
};

// the E-byte element at byte offset `off` of a word, zero- or sign-extended
template <int E, bool SIGNED>
__device__ __forceinline__ unsigned mp_elem(unsigned word, int off) {
  if constexpr (E == 1) {
    const unsigned b = (word >> ((off & 3) * 8)) & 0xFFu;
    return SIGNED ? (unsigned)(int)(signed char)b : b;
  } else if constexpr (E == 2) {
    const unsigned h = (word >> ((off & 2) * 8)) & 0xFFFFu;
    return SIGNED ? (unsigned)(int)(short)h : h;
  } else {
    return word;
  }
}
template <int W> constexpr int mp_elem_bytes() { return W < 4 ? W : 4; }
template <int W> constexpr unsigned mp_elem_mask() {
  return W == 1 ? 0xFFu : W == 2 ? 0xFFFFu : 0xFFFFFFFFu;
}

struct MpState {
  int mismatched, first_step, first_off;
  unsigned dropped, raised, checksum, sum_mask, flags;
};

__device__ __forceinline__ void mp_compare(MpState& s, unsigned got, unsigned want, unsigned emask,
                                           int gstep, int off) {
  const unsigned diff = got ^ want;
  const bool bad = diff != 0;
  const bool first = bad && (s.first_step < 0 || (s.first_step == gstep && off < s.first_off));
  s.mismatched += bad;
  s.dropped |= want & diff & emask;
  s.raised |= got & diff & emask;
  s.checksum += got & s.sum_mask;
  s.first_step = first ? gstep : s.first_step;
  s.first_off = first ? off : s.first_off;
}

// the wave's stores have reached memory and its next loads see them
__device__ __forceinline__ void mp_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mp_rsrc(const unsigned* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(base), 0, bytes, MP_RSRC_WORD3);
}

template <int W, bool SIGNED>
__device__ __forceinline__ void mp_buf_load(unsigned (&out)[4], __amdgpu_buffer_rsrc_t r, int voff,
                                            int soff) {
  if constexpr (W == 1) {
    const unsigned char b = __builtin_amdgcn_raw_buffer_load_b8(r, voff, soff, 0);
    out[0] = SIGNED ? (unsigned)(int)(signed char)b : (unsigned)b;
  } else if constexpr (W == 2) {
    const unsigned short h = __builtin_amdgcn_raw_buffer_load_b16(r, voff, soff, 0);
    out[0] = SIGNED ? (unsigned)(int)(short)h : (unsigned)h;
  } else if constexpr (W == 4) {
    out[0] = __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
  } else if constexpr (W == 8) {
    const mp_u2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
    out[0] = v.x, out[1] = v.y;
  } else if constexpr (W == 12) {
    const mp_u3 v = __builtin_amdgcn_raw_buffer_load_b96(r, voff, soff, 0);
    out[0] = v.x, out[1] = v.y, out[2] = v.z;
  } else {
    const mp_u4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    out[0] = v.x, out[1] = v.y, out[2] = v.z, out[3] = v.w;
  }
  asm volatile("" ::: "memory");
}

template <int W>
__device__ __forceinline__ void mp_buf_store(const unsigned (&d)[4], __amdgpu_buffer_rsrc_t r,
                                             int voff, int soff) {
  if constexpr (W == 1) {
    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)d[0], r, voff, soff, 0);
  } else if constexpr (W == 2) {
    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)d[0], r, voff, soff, 0);
  } else if constexpr (W == 4) {
    __builtin_amdgcn_raw_buffer_store_b32(d[0], r, voff, soff, 0);
  } else if constexpr (W == 8) {
    __builtin_amdgcn_raw_buffer_store_b64(mp_u2{d[0], d[1]}, r, voff, soff, 0);
  } else if constexpr (W == 12) {
    __builtin_amdgcn_raw_buffer_store_b96(mp_u3{d[0], d[1], d[2]}, r, voff, soff, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b128(mp_u4{d[0], d[1], d[2], d[3]}, r, voff, soff, 0);
  }
  asm volatile("" ::: "memory");
}

// W bytes at byte offset o of the row through plain typed loads and stores
template <int W>
__device__ __forceinline__ void mp_plain_load(unsigned (&out)[4], const unsigned* row, int o) {
  if constexpr (W == 1) {
    out[0] = reinterpret_cast<const unsigned char*>(row)[o];
  } else if constexpr (W == 2) {
    out[0] = reinterpret_cast<const unsigned short*>(row)[o >> 1];
  } else {
#pragma unroll
    for (int c = 0; c < W / 4; c++) out[c] = row[(o >> 2) + c];
  }
  asm volatile("" ::: "memory");
}
template <int W>
__device__ __forceinline__ void mp_plain_store(unsigned* row, int o, const unsigned (&d)[4]) {
  if constexpr (W == 1) {
    reinterpret_cast<unsigned char*>(row)[o] = (unsigned char)d[0];
  } else if constexpr (W == 2) {
    reinterpret_cast<unsigned short*>(row)[o >> 1] = (unsigned short)d[0];
  } else {
#pragma unroll
    for (int c = 0; c < W / 4; c++) row[(o >> 2) + c] = d[c];
  }
  asm volatile("" ::: "memory");
}

// the slice := v ^ x, with global_store_dwordx4
__device__ __forceinline__ void mp_fill_slice(unsigned* row, const MpPat& p, unsigned x, int lane) {
  uint4* q = reinterpret_cast<uint4*>(row);
  for (int k = lane; k < MP_SLICE_WORDS / 4; k += 64)
    q[k] = make_uint4(p.word(4 * k) ^ x, p.word(4 * k + 1) ^ x, p.word(4 * k + 2) ^ x,
                      p.word(4 * k + 3) ^ x);
  mp_fence();
}

// the slice against v ^ x, with global_load_dword
__device__ __forceinline__ void mp_check_slice(MpState& s, const unsigned* row, const MpPat& p,
                                               unsigned x, int gstep, int lane) {
  for (int k = lane; k < MP_SLICE_WORDS; k += 64) {
    const unsigned got = row[k];
    asm volatile("" ::: "memory");
    mp_compare(s, got, p.word(k) ^ x, 0xFFFFFFFFu, gstep, 4 * k);
  }
}

// lane 0 flips one bit of its wave's own row (wave-uniform `here`)
__device__ __forceinline__ void mp_flip_global(unsigned* row, bool here, int off, int bit,
                                               int lane) {
  if (here) {
    if (lane == 0) row[off >> 2] ^= 1u << (((off & 3) << 3) + bit);
    mp_fence();
  }
}
__device__ __forceinline__ void mp_flip_lds(unsigned* region, bool here, int off, int bit,
                                            int lane) {
  if (here) {
    if (lane == 0) region[off >> 2] ^= 1u << (((off & 3) << 3) + bit);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// Byte offset of access k of a lane when W-byte accesses tile the slice lane
// by lane, in batches of four: outer is wave-uniform, inner a compile-time
// constant that can become the instruction's immediate.
// SPLIT 0: voffset = lane*W + inner (imm), soffset = outer
// SPLIT 1: voffset = outer + lane*W + inner (imm), soffset = 0
// SPLIT 2: voffset = lane*W, soffset = outer + inner
template <int W, int SPLIT>
__device__ __forceinline__ void mp_split(int outer, int inner, int lane, int& voff, int& soff) {
  voff = SPLIT == 0 ? lane * W + inner : SPLIT == 1 ? outer + lane * W + inner : lane * W;
  soff = SPLIT == 0 ? outer : SPLIT == 1 ? 0 : outer + inner;
}

template <int W, bool SIGNED, int SPLIT>
__device__ __forceinline__ void mp_buf_load_step(MpState& s, __amdgpu_buffer_rsrc_t r,
                                                 const MpPat& p, int gstep, int lane) {
  constexpr int PER = MP_SLICE_BYTES / (64 * W);
  constexpr int E = mp_elem_bytes<W>();
#pragma unroll 1
  for (int k0 = 0; k0 < PER; k0 += 4) {
    unsigned got[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      int voff, soff;
      mp_split<W, SPLIT>(k0 * 64 * W, u * 64 * W, lane, voff, soff);
      mp_buf_load<W, SIGNED>(got[u], r, voff, soff);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int off = (k0 + u) * 64 * W + lane * W;
#pragma unroll
      for (int c = 0; c < W / E; c++)
        mp_compare(s, got[u][c], mp_elem<E, SIGNED>(p.word((off >> 2) + c), off),
                   mp_elem_mask<W>(), gstep, off + 4 * c);
    }
  }
}

template <int W, int SPLIT>
__device__ __forceinline__ void mp_buf_store_step(__amdgpu_buffer_rsrc_t r, const MpPat& p,
                                                  unsigned x, int lane) {
  constexpr int PER = MP_SLICE_BYTES / (64 * W);
  constexpr int E = mp_elem_bytes<W>();
#pragma unroll 1
  for (int k0 = 0; k0 < PER; k0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int off = (k0 + u) * 64 * W + lane * W;
      unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int c = 0; c < W / E; c++) d[c] = mp_elem<E, false>(p.word((off >> 2) + c) ^ x, off);
      int voff, soff;
      mp_split<W, SPLIT>(k0 * 64 * W, u * 64 * W, lane, voff, soff);
      mp_buf_store<W>(d, r, voff, soff);
    }
  }
}

struct MpInject {
  bool block_here, wave_here;  // the injected block; its wave 0
  int step, offset, bit;
};

// --- section buf ---
__device__ __forceinline__ void mp_section_buf(MpState& s, unsigned* row, const MpPat& p,
                                               int gbase, const MpInject& inj, int lane) {
  const __amdgpu_buffer_rsrc_t r = mp_rsrc(row, MP_SLICE_BYTES);
  mp_fill_slice(row, p, 0u, lane);
#define MP_BUF_LOAD(STEP, W, SIGNED, SPLIT)                                    \
  {                                                                            \
    const bool here = inj.wave_here && inj.step == gbase + (STEP);             \
    mp_flip_global(row, here, inj.offset, inj.bit, lane);                      \
    mp_buf_load_step<W, SIGNED, SPLIT>(s, r, p, gbase + (STEP), lane);         \
    mp_flip_global(row, here, inj.offset, inj.bit, lane);                      \
  }
  MP_BUF_LOAD(0, 1, false, 0)
  MP_BUF_LOAD(1, 1, true, 1)
  MP_BUF_LOAD(2, 2, false, 2)
  MP_BUF_LOAD(3, 2, true, 0)
  MP_BUF_LOAD(4, 4, false, 1)
  MP_BUF_LOAD(5, 8, false, 2)
  MP_BUF_LOAD(6, 12, false, 0)
  MP_BUF_LOAD(7, 16, false, 1)
#undef MP_BUF_LOAD
#define MP_BUF_STORE(STEP, W, SPLIT)                                                         \
  {                                                                                          \
    const unsigned x = (unsigned)((STEP) + 1) * 0x9E3779B9u;                                 \
    mp_buf_store_step<W, SPLIT>(r, p, x, lane);                                              \
    mp_fence();                                                                              \
    mp_flip_global(row, inj.wave_here && inj.step == gbase + (STEP), inj.offset, inj.bit, lane); \
    mp_check_slice(s, row, p, x, gbase + (STEP), lane);                                      \
  }
  MP_BUF_STORE(8, 1, 1)
  MP_BUF_STORE(9, 2, 0)
  MP_BUF_STORE(10, 4, 2)
  MP_BUF_STORE(11, 8, 1)
  MP_BUF_STORE(12, 12, 2)
  MP_BUF_STORE(13, 16, 0)
#undef MP_BUF_STORE
}

// --- section oob ---
template <int W>
__device__ __forceinline__ void mp_oob_load_step(MpState& s, const unsigned* row, const MpPat& p,
                                                 int L, bool lengthen, int gstep, int lane) {
  constexpr int E = mp_elem_bytes<W>();
  const __amdgpu_buffer_rsrc_t r = mp_rsrc(row, lengthen ? mp_oob_first_out(L, W) + W : L);
  const int o = mp_oob_lo(L, W) + lane * W;
  const bool in = o + W <= L, out = o >= L;
  if (lane < MP_OOB_LANES && (in || out)) {  // a straddling access is never issued
    unsigned got[4];
    mp_buf_load<W, false>(got, r, o, 0);
#pragma unroll
    for (int c = 0; c < W / E; c++)
      mp_compare(s, got[c], in ? mp_elem<E, false>(p.word((o >> 2) + c), o) : 0u,
                 mp_elem_mask<W>(), gstep, o + 4 * c);
  }
}

template <int W>
__device__ __forceinline__ void mp_oob_store_step(MpState& s, unsigned* row, const MpPat& p, int L,
                                                  bool lengthen, int step, int gstep, int lane) {
  constexpr int E = mp_elem_bytes<W>();
  const __amdgpu_buffer_rsrc_t r = mp_rsrc(row, lengthen ? mp_oob_first_out(L, W) + W : L);
  const unsigned x = (unsigned)(step + 1) * 0x9E3779B9u;
  const int o = mp_oob_lo(L, W) + lane * W;
  const bool in = o + W <= L, out = o >= L;
  const bool active = lane < MP_OOB_LANES && (in || out);
  unsigned was[4] = {0u, 0u, 0u, 0u}, want[4] = {0u, 0u, 0u, 0u};
  if (active) {
    unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < W / E; c++) {
      was[c] = mp_elem<E, false>(p.row_word((o >> 2) + c), o);
      // in range: the neighbours must land; out of range: a marker that must not
      d[c] = in ? mp_elem<E, false>(p.word((o >> 2) + c) ^ x, o)
                : mp_elem<E, false>(MP_OOB_MARKER, o);
      want[c] = in ? d[c] : was[c];
    }
    mp_buf_store<W>(d, r, o, 0);
  }
  mp_fence();
  if (active) {
    unsigned got[4];
    mp_plain_load<W>(got, row, o);
#pragma unroll
    for (int c = 0; c < W / E; c++)
      mp_compare(s, got[c], want[c], mp_elem_mask<W>(), gstep, o + 4 * c);
    mp_plain_store<W>(row, o, was);  // the row as it stood
  }
  mp_fence();
}

__device__ __forceinline__ void mp_section_oob(MpState& s, unsigned* row, const MpPat& p,
                                               int gbase, const MpInject& inj, int lane) {
  mp_fill_slice(row, p, 0u, lane);
  for (int li = 0; li < 5; li++) {
    const int L = mp_oob_length(li);
    const int step0 = li * 12;
#define MP_OOB_PAIR(K, W)                                                                  \
  mp_oob_load_step<W>(s, row, p, L, inj.block_here && inj.step == gbase + step0 + (K),     \
                      gbase + step0 + (K), lane);                                          \
  mp_oob_store_step<W>(s, row, p, L, inj.block_here && inj.step == gbase + step0 + 6 + (K), \
                       step0 + 6 + (K), gbase + step0 + 6 + (K), lane);
    MP_OOB_PAIR(0, 1)
    MP_OOB_PAIR(1, 2)
    MP_OOB_PAIR(2, 4)
    MP_OOB_PAIR(3, 8)
    MP_OOB_PAIR(4, 12)
    MP_OOB_PAIR(5, 16)
#undef MP_OOB_PAIR
  }
  // the guard, with plain loads: no out-of-range store may have reached it
  const unsigned got = row[MP_SLICE_WORDS + lane];
  asm volatile("" ::: "memory");
  mp_compare(s, got, MP_GUARD_SENTINEL, 0xFFFFFFFFu, gbase + 60, MP_SLICE_BYTES + 4 * lane);
}

// --- section lds ---
// N bytes per lane; BUF: through the descriptor, else global_load_lds. With
// oob_lanes > 0 a single issue whose descriptor covers only the lanes below.
template <int N, bool BUF>
__device__ __forceinline__ void mp_lds_step(MpState& s, unsigned* region, const unsigned* row,
                                            const MpPat& p, int dst, int inrange, int gstep,
                                            const MpInject& inj, int lane) {
  uint4* q = reinterpret_cast<uint4*>(region);
  for (int k = lane; k < MP_LDS_WAVE_WORDS / 4; k += 64)
    q[k] = make_uint4(MP_LDS_SENTINEL, MP_LDS_SENTINEL, MP_LDS_SENTINEL, MP_LDS_SENTINEL);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  MP_LDS_AS unsigned* to = (MP_LDS_AS unsigned*)region + dst / 4;
  int moved = MP_SLICE_WORDS;
  if (inrange > 0) {
    // addresses stay inside the row; lanes >= inrange are beyond the length
    __builtin_amdgcn_raw_ptr_buffer_load_lds(mp_rsrc(row, 4 * inrange), to, 4, lane * 4, 0, 0, 0);
    moved = 64;
  } else {
    constexpr int CHUNK = 64 * N;
    const __amdgpu_buffer_rsrc_t r = mp_rsrc(row, MP_SLICE_BYTES);
#pragma unroll 1
    for (int k0 = 0; k0 < MP_SLICE_BYTES / CHUNK; k0 += 4) {
      MP_LDS_AS unsigned* to_k = to + k0 * (CHUNK / 4);  // wave-uniform: goes to M0
      const int voff = k0 * CHUNK + lane * N;
      const auto* from =
          (__attribute__((address_space(1))) const unsigned*)(row + (k0 * CHUNK + lane * N) / 4);
      // the size and the immediate must be literals for the builtins
#define MP_LDS_ISSUE(SIZE, IMM)                                                   \
  if constexpr (BUF)                                                              \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, to_k, SIZE, voff, 0, IMM, 0);     \
  else                                                                            \
    __builtin_amdgcn_global_load_lds(from, to_k, SIZE, IMM, 0);
#define MP_LDS_ISSUE4(SIZE)                                                       \
  MP_LDS_ISSUE(SIZE, 0)                                                           \
  MP_LDS_ISSUE(SIZE, 64 * SIZE) MP_LDS_ISSUE(SIZE, 128 * SIZE) MP_LDS_ISSUE(SIZE, 192 * SIZE)
      if constexpr (N == 4) {
        MP_LDS_ISSUE4(4)
      } else if constexpr (N == 12) {
        MP_LDS_ISSUE4(12)
      } else {
        MP_LDS_ISSUE4(16)
      }
#undef MP_LDS_ISSUE4
#undef MP_LDS_ISSUE
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  mp_flip_lds(region, inj.wave_here && inj.step == gstep, inj.offset, inj.bit, lane);
  for (int k = lane; k < MP_LDS_WAVE_WORDS / 4; k += 64) {
    const uint4 v = q[k];
    const unsigned got[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int i = 4 * k + c - dst / 4;  // the slice word that belongs here
      if (inrange > 0 && i >= inrange && i < moved) {
        // unknown: 0 written or the sentinel left; anything else is a mismatch
        if (got[c] == 0u) s.flags |= 1u;
        else if (got[c] == MP_LDS_SENTINEL) s.flags |= 2u;
        else mp_compare(s, got[c], MP_LDS_SENTINEL, 0xFFFFFFFFu, gstep, 16 * k + 4 * c);
      } else {
        const bool copied = i >= 0 && i < (inrange > 0 ? inrange : moved);
        mp_compare(s, got[c], copied ? p.word(i) : MP_LDS_SENTINEL, 0xFFFFFFFFu, gstep,
                   16 * k + 4 * c);
      }
    }
  }
}

__device__ __forceinline__ void mp_section_lds(MpState& s, unsigned* region, unsigned* row,
                                               const MpPat& p, int gbase, const MpInject& inj,
                                               int lane) {
  mp_fill_slice(row, p, 0u, lane);
  // no dwordx3 step: measured on an MI355X, lane l's 12 bytes do not land at
  // base + l*12 (BENCHMARKS.md "Memory-path probe"), and no description of
  // another layout is at hand to write a mirror from
  mp_lds_step<4, false>(s, region, row, p, mp_lds_dst(0), 0, gbase + 0, inj, lane);
  mp_lds_step<16, false>(s, region, row, p, mp_lds_dst(1), 0, gbase + 1, inj, lane);
  mp_lds_step<4, true>(s, region, row, p, mp_lds_dst(2), 0, gbase + 2, inj, lane);
  mp_lds_step<16, true>(s, region, row, p, mp_lds_dst(3), 0, gbase + 3, inj, lane);
  mp_lds_step<4, true>(s, region, row, p, mp_lds_dst(4), MP_LDS_OOB_INRANGE, gbase + 4, inj, lane);
}

// --- section forms ---
// A d16 load writes one half of its register. Four loads per asm, the register
// preset to a canary; the loaded half is compared, and whether the other half
// survived is recorded in field [7], not judged: LLVM documents that the unused
// bits are not preserved where SRAM ECC is on (d16PreservesUnusedBits), as on
// the MI355X, where they read back zero.
#define MP_D16_LOAD4(INSTR, ADDR, SFX, STRIDE, R)                                         \
  asm volatile(INSTR " %0, %4" SFX " offset:0\n\t" INSTR " %1, %4" SFX " offset:%5\n\t"  \
               INSTR " %2, %4" SFX " offset:%6\n\t" INSTR " %3, %4" SFX " offset:%7\n\t" \
               "s_waitcnt vmcnt(0) lgkmcnt(0)"                                            \
               : "+v"(R[0]), "+v"(R[1]), "+v"(R[2]), "+v"(R[3])                           \
               : "v"(ADDR), "n"(STRIDE), "n"(2 * (STRIDE)), "n"(3 * (STRIDE))             \
               : "memory")
#define MP_D16_STORE4(INSTR, ADDR, SFX, STRIDE, R)                                        \
  asm volatile(INSTR " %4, %0" SFX " offset:0\n\t" INSTR " %4, %1" SFX " offset:%5\n\t"  \
               INSTR " %4, %2" SFX " offset:%6\n\t" INSTR " %4, %3" SFX " offset:%7"    \
               :                                                                          \
               : "v"(R[0]), "v"(R[1]), "v"(R[2]), "v"(R[3]), "v"(ADDR), "n"(STRIDE),      \
                 "n"(2 * (STRIDE)), "n"(3 * (STRIDE))                                     \
               : "memory")

enum { MP_F_PLAIN = 0, MP_F_D16, MP_F_D16_HI };

// One pass over the 12288 B at `base` (the slice, or the wave's LDS region) in
// E-byte elements, lane by lane, four per batch; FORM says how each is loaded.
template <bool LDS, int E, bool SIGNED, int FORM>
__device__ __forceinline__ void mp_narrow_load_step(MpState& s, const unsigned* base,
                                                    const MpPat& p, int gstep, int lane) {
  constexpr int PER = MP_SLICE_BYTES / (64 * E);
  constexpr int STRIDE = 64 * E;
  const unsigned char* bytes = reinterpret_cast<const unsigned char*>(base);
#pragma unroll 1
  for (int k0 = 0; k0 < PER; k0 += 4) {
    const int off0 = k0 * STRIDE + lane * E;
    unsigned got[4] = {MP_D16_CANARY, MP_D16_CANARY, MP_D16_CANARY, MP_D16_CANARY};
    if constexpr (FORM == MP_F_PLAIN) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const unsigned char* a = bytes + off0 + u * STRIDE;
        if constexpr (E == 1)
          got[u] = SIGNED ? (unsigned)(int)*reinterpret_cast<const signed char*>(a) : (unsigned)*a;
        else
          got[u] = SIGNED ? (unsigned)(int)*reinterpret_cast<const short*>(a)
                          : (unsigned)*reinterpret_cast<const unsigned short*>(a);
        asm volatile("" ::: "memory");
      }
    } else if constexpr (LDS) {
      const unsigned a = (unsigned)(size_t)(MP_LDS_AS const unsigned char*)(bytes + off0);
      if constexpr (E == 1 && !SIGNED && FORM == MP_F_D16) MP_D16_LOAD4("ds_read_u8_d16", a, "", STRIDE, got);
      if constexpr (E == 1 && !SIGNED && FORM == MP_F_D16_HI) MP_D16_LOAD4("ds_read_u8_d16_hi", a, "", STRIDE, got);
      if constexpr (E == 1 && SIGNED && FORM == MP_F_D16) MP_D16_LOAD4("ds_read_i8_d16", a, "", STRIDE, got);
      if constexpr (E == 1 && SIGNED && FORM == MP_F_D16_HI) MP_D16_LOAD4("ds_read_i8_d16_hi", a, "", STRIDE, got);
      if constexpr (E == 2 && FORM == MP_F_D16) MP_D16_LOAD4("ds_read_u16_d16", a, "", STRIDE, got);
      if constexpr (E == 2 && FORM == MP_F_D16_HI) MP_D16_LOAD4("ds_read_u16_d16_hi", a, "", STRIDE, got);
    } else {
      const unsigned char* a = bytes + off0;
      if constexpr (E == 1 && !SIGNED && FORM == MP_F_D16) MP_D16_LOAD4("global_load_ubyte_d16", a, ", off", STRIDE, got);
      if constexpr (E == 1 && !SIGNED && FORM == MP_F_D16_HI) MP_D16_LOAD4("global_load_ubyte_d16_hi", a, ", off", STRIDE, got);
      if constexpr (E == 1 && SIGNED && FORM == MP_F_D16) MP_D16_LOAD4("global_load_sbyte_d16", a, ", off", STRIDE, got);
      if constexpr (E == 1 && SIGNED && FORM == MP_F_D16_HI) MP_D16_LOAD4("global_load_sbyte_d16_hi", a, ", off", STRIDE, got);
      if constexpr (E == 2 && FORM == MP_F_D16) MP_D16_LOAD4("global_load_short_d16", a, ", off", STRIDE, got);
      if constexpr (E == 2 && FORM == MP_F_D16_HI) MP_D16_LOAD4("global_load_short_d16_hi", a, ", off", STRIDE, got);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int off = off0 + u * STRIDE;
      unsigned want = mp_elem<E, SIGNED>(p.word(off >> 2), off), g = got[u];
      if constexpr (FORM != MP_F_PLAIN) {
        // the element, extended to 16 bits, is judged; what became of the
        // other half (the canary) is recorded: 1 kept, 2 zeroed, 4 neither
        const unsigned other = FORM == MP_F_D16 ? g >> 16 : g & 0xFFFFu;
        const unsigned canary = FORM == MP_F_D16 ? MP_D16_CANARY >> 16 : MP_D16_CANARY & 0xFFFFu;
        s.flags |= other == canary ? 1u : other == 0u ? 2u : 4u;
        g = FORM == MP_F_D16 ? g & 0xFFFFu : g >> 16;
        want &= 0xFFFFu;
      }
      mp_compare(s, g, want, mp_elem_mask<E>(), gstep, off);
    }
  }
}

// the 12288 B at `base` := v ^ x in E-byte elements; HI: from the high half of
// a register whose low half holds the complement
template <bool LDS, int E, bool HI>
__device__ __forceinline__ void mp_narrow_store_step(unsigned* base, const MpPat& p, unsigned x,
                                                     int lane) {
  constexpr int PER = MP_SLICE_BYTES / (64 * E);
  constexpr int STRIDE = 64 * E;
  unsigned char* bytes = reinterpret_cast<unsigned char*>(base);
#pragma unroll 1
  for (int k0 = 0; k0 < PER; k0 += 4) {
    const int off0 = k0 * STRIDE + lane * E;
    unsigned d[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int off = off0 + u * STRIDE;
      const unsigned e = mp_elem<E, false>(p.word(off >> 2) ^ x, off);
      d[u] = HI ? (e << 16) | (~e & 0xFFFFu) : e | (~e << 16);
    }
    if constexpr (LDS) {
      const unsigned a = (unsigned)(size_t)(MP_LDS_AS unsigned char*)(bytes + off0);
      if constexpr (E == 1 && !HI) MP_D16_STORE4("ds_write_b8", a, "", STRIDE, d);
      if constexpr (E == 1 && HI) MP_D16_STORE4("ds_write_b8_d16_hi", a, "", STRIDE, d);
      if constexpr (E == 2 && !HI) MP_D16_STORE4("ds_write_b16", a, "", STRIDE, d);
      if constexpr (E == 2 && HI) MP_D16_STORE4("ds_write_b16_d16_hi", a, "", STRIDE, d);
    } else {
      unsigned char* a = bytes + off0;
      if constexpr (E == 1 && !HI) MP_D16_STORE4("global_store_byte", a, ", off", STRIDE, d);
      if constexpr (E == 1 && HI) MP_D16_STORE4("global_store_byte_d16_hi", a, ", off", STRIDE, d);
      if constexpr (E == 2 && !HI) MP_D16_STORE4("global_store_short", a, ", off", STRIDE, d);
      if constexpr (E == 2 && HI) MP_D16_STORE4("global_store_short_d16_hi", a, ", off", STRIDE, d);
    }
  }
}

// the first 12288 B of the LDS region := v ^ x with ds_write_b32, and the same
// against v ^ x with ds_read_b128
__device__ __forceinline__ void mp_fill_lds(unsigned* region, const MpPat& p, unsigned x, int lane) {
  for (int k = lane; k < MP_SLICE_WORDS; k += 64) {
    region[k] = p.word(k) ^ x;
    asm volatile("" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void mp_check_lds(MpState& s, const unsigned* region, const MpPat& p,
                                             unsigned x, int gstep, int lane) {
  const uint4* q = reinterpret_cast<const uint4*>(region);
  for (int k = lane; k < MP_SLICE_WORDS / 4; k += 64) {
    const uint4 v = q[k];
    asm volatile("" ::: "memory");
    mp_compare(s, v.x, p.word(4 * k) ^ x, 0xFFFFFFFFu, gstep, 16 * k);
    mp_compare(s, v.y, p.word(4 * k + 1) ^ x, 0xFFFFFFFFu, gstep, 16 * k + 4);
    mp_compare(s, v.z, p.word(4 * k + 2) ^ x, 0xFFFFFFFFu, gstep, 16 * k + 8);
    mp_compare(s, v.w, p.word(4 * k + 3) ^ x, 0xFFFFFFFFu, gstep, 16 * k + 12);
  }
}

// Wide LDS forms. Each visits the 3072 words once; WIDE names the form:
//   0 b64, 1 b96 on 16 B aligned quads with the fourth word through b32, 2 b128
//   3 read2/write2_b32       words i and i+64   (offset1:64, units of 4 B)
//   4 read2st64/write2st64   words i and i+384  (offset1:6, units of 256 B)
//   5 read2/write2_b64       words i,i+1 and i+128,i+129 (offset1:64, units of 8 B)
// `first[j]`: the word index of access j's first word for this lane; the other
// words follow by the form.
template <int WIDE> struct MpWide;
template <> struct MpWide<0> { static constexpr int N = 24, WORDS = 2;
  __device__ static int first(int j, int lane) { return 2 * (j * 64 + lane); }
  __device__ static int word(int c) { return c; } };
template <> struct MpWide<1> { static constexpr int N = 12, WORDS = 4;  // b96, and b32 for the 4th
  __device__ static int first(int j, int lane) { return 4 * (j * 64 + lane); }
  __device__ static int word(int c) { return c; } };
template <> struct MpWide<2> { static constexpr int N = 12, WORDS = 4;
  __device__ static int first(int j, int lane) { return 4 * (j * 64 + lane); }
  __device__ static int word(int c) { return c; } };
template <> struct MpWide<3> { static constexpr int N = 24, WORDS = 2;
  __device__ static int first(int j, int lane) { return j * 128 + lane; }
  __device__ static int word(int c) { return 64 * c; } };
template <> struct MpWide<4> { static constexpr int N = 24, WORDS = 2;
  __device__ static int first(int j, int lane) { return (j / 6) * 768 + (j % 6) * 64 + lane; }
  __device__ static int word(int c) { return 384 * c; } };
template <> struct MpWide<5> { static constexpr int N = 12, WORDS = 4;
  __device__ static int first(int j, int lane) { return j * 256 + 2 * lane; }
  __device__ static int word(int c) { return (c & 1) + 128 * (c >> 1); } };

template <int WIDE>
__device__ __forceinline__ void mp_wide_read_step(MpState& s, const unsigned* region,
                                                  const MpPat& p, int gstep, int lane) {
  using F = MpWide<WIDE>;
#pragma unroll 1
  for (int j = 0; j < F::N; j++) {
    const int i0 = F::first(j, lane);
    const unsigned a = (unsigned)(size_t)(MP_LDS_AS const unsigned*)(region + i0);
    unsigned got[4] = {0u, 0u, 0u, 0u};
    if constexpr (WIDE == 0) {
      mp_u2 v;
      asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
      got[0] = v.x, got[1] = v.y;
    } else if constexpr (WIDE == 1) {
      mp_u3 v;
      asm volatile("ds_read_b96 %0, %2\n\tds_read_b32 %1, %2 offset:12\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(v), "=&v"(got[3]) : "v"(a) : "memory");
      got[0] = v.x, got[1] = v.y, got[2] = v.z;
    } else if constexpr (WIDE == 3 || WIDE == 4) {
      mp_u2 v;
      if constexpr (WIDE == 3)
        asm volatile("ds_read2_b32 %0, %1 offset1:64\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
      else
        asm volatile("ds_read2st64_b32 %0, %1 offset1:6\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
      got[0] = v.x, got[1] = v.y;
    } else {
      mp_u4 v;
      asm volatile("ds_read2_b64 %0, %1 offset1:64\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
      got[0] = v.x, got[1] = v.y, got[2] = v.z, got[3] = v.w;
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int c = 0; c < F::WORDS; c++) {
      const int i = i0 + F::word(c);
      mp_compare(s, got[c], p.word(i), 0xFFFFFFFFu, gstep, 4 * i);
    }
  }
}

template <int WIDE>
__device__ __forceinline__ void mp_wide_write_step(unsigned* region, const MpPat& p, unsigned x,
                                                   int lane) {
  using F = MpWide<WIDE>;
#pragma unroll 1
  for (int j = 0; j < F::N; j++) {
    const int i0 = F::first(j, lane);
    const unsigned a = (unsigned)(size_t)(MP_LDS_AS unsigned*)(region + i0);
    unsigned d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < F::WORDS; c++) d[c] = p.word(i0 + F::word(c)) ^ x;
    if constexpr (WIDE == 0) {
      asm volatile("ds_write_b64 %0, %1" : : "v"(a), "v"(mp_u2{d[0], d[1]}) : "memory");
    } else if constexpr (WIDE == 1) {
      asm volatile("ds_write_b96 %0, %1\n\tds_write_b32 %0, %2 offset:12"
                   : : "v"(a), "v"(mp_u3{d[0], d[1], d[2]}), "v"(d[3]) : "memory");
    } else if constexpr (WIDE == 2) {
      asm volatile("ds_write_b128 %0, %1" : : "v"(a), "v"(mp_u4{d[0], d[1], d[2], d[3]}) : "memory");
    } else if constexpr (WIDE == 3) {
      asm volatile("ds_write2_b32 %0, %1, %2 offset1:64" : : "v"(a), "v"(d[0]), "v"(d[1]) : "memory");
    } else if constexpr (WIDE == 4) {
      asm volatile("ds_write2st64_b32 %0, %1, %2 offset1:6" : : "v"(a), "v"(d[0]), "v"(d[1]) : "memory");
    } else {
      asm volatile("ds_write2_b64 %0, %1, %2 offset1:64"
                   : : "v"(a), "v"(mp_u2{d[0], d[1]}), "v"(mp_u2{d[2], d[3]}) : "memory");
    }
    asm volatile("" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__device__ __forceinline__ void mp_section_forms(MpState& s, unsigned* region, unsigned* row,
                                                 const MpPat& p, int gbase, const MpInject& inj,
                                                 int lane) {
  int step = 0;
  mp_fill_slice(row, p, 0u, lane);
  mp_fill_lds(region, p, 0u, lane);
#define MP_HERE (inj.wave_here && inj.step == gbase + step)
#define MP_GLOAD(E, SIGNED, FORM)                                                      \
  {                                                                                    \
    const bool here = MP_HERE;                                                         \
    mp_flip_global(row, here, inj.offset, inj.bit, lane);                              \
    mp_narrow_load_step<false, E, SIGNED, FORM>(s, row, p, gbase + step, lane);        \
    mp_flip_global(row, here, inj.offset, inj.bit, lane);                              \
    step++;                                                                            \
  }
#define MP_GSTORE(E, HI)                                                               \
  {                                                                                    \
    const unsigned x = (unsigned)(step + 1) * 0x9E3779B9u;                             \
    mp_narrow_store_step<false, E, HI>(row, p, x, lane);                               \
    mp_fence();                                                                        \
    mp_flip_global(row, MP_HERE, inj.offset, inj.bit, lane);                           \
    mp_check_slice(s, row, p, x, gbase + step, lane);                                  \
    step++;                                                                            \
  }
#define MP_LREAD(CALL)                                                                 \
  {                                                                                    \
    const bool here = MP_HERE;                                                         \
    mp_flip_lds(region, here, inj.offset, inj.bit, lane);                              \
    CALL;                                                                              \
    mp_flip_lds(region, here, inj.offset, inj.bit, lane);                              \
    step++;                                                                            \
  }
#define MP_LWRITE(CALL)                                                                \
  {                                                                                    \
    const unsigned x = (unsigned)(step + 1) * 0x9E3779B9u;                             \
    CALL;                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                 \
    mp_flip_lds(region, MP_HERE, inj.offset, inj.bit, lane);                           \
    mp_check_lds(s, region, p, x, gbase + step, lane);                                 \
    step++;                                                                            \
  }
  // global path: steps 0..13
  MP_GLOAD(1, false, MP_F_PLAIN)
  MP_GLOAD(1, true, MP_F_PLAIN)
  MP_GLOAD(2, false, MP_F_PLAIN)
  MP_GLOAD(2, true, MP_F_PLAIN)
  MP_GLOAD(1, false, MP_F_D16)
  MP_GLOAD(1, false, MP_F_D16_HI)
  MP_GLOAD(1, true, MP_F_D16)
  MP_GLOAD(1, true, MP_F_D16_HI)
  MP_GLOAD(2, false, MP_F_D16)
  MP_GLOAD(2, false, MP_F_D16_HI)
  MP_GSTORE(1, false)
  MP_GSTORE(1, true)
  MP_GSTORE(2, false)
  MP_GSTORE(2, true)
  // LDS reads: steps 14..28
  MP_LREAD((mp_narrow_load_step<true, 1, false, MP_F_PLAIN>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 1, true, MP_F_PLAIN>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 2, false, MP_F_PLAIN>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 2, true, MP_F_PLAIN>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 1, false, MP_F_D16>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 1, false, MP_F_D16_HI>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 1, true, MP_F_D16>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 1, true, MP_F_D16_HI>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 2, false, MP_F_D16>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_narrow_load_step<true, 2, false, MP_F_D16_HI>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_wide_read_step<0>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_wide_read_step<1>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_wide_read_step<3>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_wide_read_step<4>(s, region, p, gbase + step, lane)))
  MP_LREAD((mp_wide_read_step<5>(s, region, p, gbase + step, lane)))
  // LDS writes: steps 29..38
  MP_LWRITE((mp_narrow_store_step<true, 1, false>(region, p, x, lane)))
  MP_LWRITE((mp_narrow_store_step<true, 2, false>(region, p, x, lane)))
  MP_LWRITE((mp_narrow_store_step<true, 1, true>(region, p, x, lane)))
  MP_LWRITE((mp_narrow_store_step<true, 2, true>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<0>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<1>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<2>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<3>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<4>(region, p, x, lane)))
  MP_LWRITE((mp_wide_write_step<5>(region, p, x, lane)))
#undef MP_HERE
#undef MP_GLOAD
#undef MP_GSTORE
#undef MP_LREAD
#undef MP_LWRITE
}

template <int SEC>
__global__ void __launch_bounds__(256)
mempath_kernel(int4* __restrict__ records, unsigned* rows, int rounds, unsigned seed,
               int inject_block, int inject_step, int inject_offset, int inject_bit) {
  constexpr bool USES_LDS = SEC == MP_LDS || SEC == MP_FORMS;
  __shared__ __attribute__((aligned(16))) unsigned lds[USES_LDS ? 4 * MP_LDS_WAVE_WORDS : 4];
  const int lane = threadIdx.x & 63;
  const int wave = uniform_wave_index();
  const unsigned place = hw_word();
  unsigned* row = rows + (size_t)wave * MP_ROW_WORDS;
  unsigned* region = lds + (USES_LDS ? (wave & 3) * MP_LDS_WAVE_WORDS : 0);
  const bool block_here = (int)blockIdx.x == inject_block;
  const MpInject inj = {block_here, block_here && (wave & 3) == 0, inject_step, inject_offset,
                        inject_bit};

  row[MP_SLICE_WORDS + lane] = MP_GUARD_SENTINEL;  // MP_GUARD_WORDS == 64 lanes
  MpState s = {0, -1, -1, 0u, 0u, 0u, 0u, 0u};
  for (int round = 0; round < rounds; round++) {
    const MpPat p = {seed + (unsigned)round * 0x9E3779B9u + (unsigned)wave * 0x7F4A7C15u,
                     (round & 1) ? 0xFFFFFFFFu : 0u};
    s.sum_mask = (round & 1) ? 0u : 0xFFFFFFFFu;
    constexpr int NSTEPS = MP_STEPS[SEC];
    const int gbase = round * NSTEPS;
    if constexpr (SEC == MP_BUF) mp_section_buf(s, row, p, gbase, inj, lane);
    if constexpr (SEC == MP_OOB) mp_section_oob(s, row, p, gbase, inj, lane);
    if constexpr (SEC == MP_LDS) mp_section_lds(s, region, row, p, gbase, inj, lane);
    if constexpr (SEC == MP_FORMS) mp_section_forms(s, region, row, p, gbase, inj, lane);
  }
  const int mismatched = (int)wave_add((unsigned)s.mismatched);
  const unsigned dropped = wave_or(s.dropped), raised = wave_or(s.raised);
  const unsigned checksum = wave_add(s.checksum), flags = wave_or(s.flags);
  // -1 as unsigned is the largest value: the earliest step, then the lowest
  // offset among the lanes that failed in that step
  const unsigned first_step = wave_min((unsigned)s.first_step);
  const unsigned first_off =
      wave_min((unsigned)s.first_step == first_step ? (unsigned)s.first_off : 0xFFFFFFFFu);
  if (lane == 0)
    store_record8(records, wave, (int)place, mismatched, (int)first_step, (int)first_off,
                  (int)dropped, (int)raised, (int)checksum, (int)flags);
}

static int mempath_section_id(const std::string& section) {
  static const char* names[MP_SECTIONS] = {"buf", "oob", "lds", "forms"};
  for (int i = 0; i < MP_SECTIONS; i++)
    if (section == names[i]) return i;
  TORCH_CHECK(false, "mempath_probe: unknown section '", section, "' (buf|oob|lds|forms)");
  return -1;
}

// One untimed warm-up launch, then one timed launch (warm_then_timed_ms); the
// kernel rewrites the guard and the slice itself, so both start alike.
// Returns (records [blocks*4, 8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> mempath_probe(const std::string& section, long blocks,
                                                long rounds, long seed, long inject_block,
                                                long inject_step, long inject_offset,
                                                long inject_bit) {
  const int sec = mempath_section_id(section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  // bounded run: a round of one workgroup measures ~1.0 ms in the oob section
  // (61 steps of a few accesses, each behind two fences), ~0.3 ms in buf,
  // ~0.5 ms in forms and ~0.05 ms in lds on an MI355X (BENCHMARKS.md
  // "Memory-path probe"); it is latency, so a full GPU of 1024 workgroups
  // amortises the oob round to ~4 us and puts 2^16 block-rounds at ~0.26 s
  TORCH_CHECK(rounds <= (1L << 16) && blocks * rounds <= (1L << 16),
              "blocks*rounds must be <= 2^16");
  // the injected element: in the slice, or for the LDS steps in the wave's region
  const long span = sec == MP_LDS ? 4L * MP_LDS_WAVE_WORDS : MP_SLICE_BYTES;
  TORCH_CHECK(inject_block >= -1 && inject_block < blocks, "inject_block out of range");
  TORCH_CHECK(inject_step >= -1 && inject_step < rounds * MP_STEPS[sec],
              "inject_step out of range");
  TORCH_CHECK(inject_offset >= -1 && inject_offset < span, "inject_offset out of range");
  TORCH_CHECK(inject_bit >= 0 && inject_bit < 32 && (inject_offset & 3) * 8 + inject_bit < 32,
              "inject_bit out of range");
  TORCH_CHECK(inject_block < 0 || sec == MP_OOB || (inject_step >= 0 && inject_offset >= 0),
              "an injection needs inject_step and inject_offset");
  if (inject_block >= 0 && inject_offset < 0) inject_offset = 0;  // oob: unused
  const long waves = blocks * 4;
  auto rows = torch::empty({waves, (long)MP_ROW_WORDS},
                           torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA));
  auto records = zero_records(waves, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<MP_SECTIONS>(sec, [&](auto s) {
      hipLaunchKernelGGL(mempath_kernel<decltype(s)::value>, dim3(blocks), dim3(256), 0, stream,
                         reinterpret_cast<int4*>(records.data_ptr<int>()),
                         reinterpret_cast<unsigned*>(rows.data_ptr<int>()), (int)rounds,
                         (unsigned)seed, (int)inject_block, (int)inject_step, (int)inject_offset,
                         (int)inject_bit);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// Conversion probe: the gfx950 narrow-format converters, which quantise to
// fp8 / fp6 / fp4 on the way into the MFMA and dequantise on the way out and
// which no probe above issues. Two kernels: cvt_sweep walks a host-built table
// of operands through one instruction form and compares every result bitwise;
// cvt_burn is the sustained register-only run in the VALU burn's shape. The
// host mirror is ops/cvt_probe.py.
//
// A path is one instruction form (CVT_PATH_NAMES, index-aligned with
// CvtPathTypes). Formats are OCP: fp8 = e4m3, bf8 = e5m2, fp6 = e2m3,
// bf6 = e3m2, fp4 = e2m1. What the instructions do, measured on an MI355X
// (BENCHMARKS.md "Conversion probe"):
//   scale   an f32 operand of which only the exponent is used; an encode
//           converts src / 2^s, a decode returns value * 2^s
//   pk 8    v_cvt_scalef32_pk_{fp8,bf8}_{f32,f16,bf16}, v_cvt_pk_{fp8,bf8}_f32:
//           two codes, src0 in the low byte, into the half of the destination
//           the word select names; the other half keeps `old`
//   pk 4    v_cvt_scalef32_pk_fp4_*: two codes, src0 in the low nibble, into
//           the byte the select names; the other three bytes keep `old`
//   fp6     v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 takes two 16-element sources
//           and INTERLEAVES them: code 2i is src0[i], code 2i+1 is src1[i], six
//           bits apiece from bit 0 of the first dword, the packing mx_pack feeds
//           the MFMA. The kernel passes elements 0,2,4.. as src0 and 1,3,5.. as
//           src1, so a table entry's 32 values come out in their own order.
//           v_cvt_scalef32_pk32_f32_{fp6,bf6} and the sr_pk32 forms take one
//           32-element operand in plain order.
//   decode  pk forms read the half (8-bit) or byte (fp4) the select names, the
//           low code first; the byte-select forms read one byte
//   sr      v_cvt_scalef32_sr_* and v_cvt_sr_*_f32 round to one of the two
//           neighbours by a random word: an exactly representable input gives
//           its own code whatever the word. They keep `old` outside the byte
//           they write and that is checked (sr_pk_fp4 through assembly, see
//           CvtSr4)
// Every value of every select is its own `if constexpr` arm and every entry
// runs through all of them. `old` is fmix32(entry * 0x9E3779B1 + 0x85EBCA6B);
// an exact path's expected dword holds old's bits outside the written field,
// so a converter that disturbs the preserved part mismatches like a wrong code.
//
// Table: `entries` packs. Entry e is IN dwords of `inputs` (wide values for an
// encode, packed codes for a decode), scales[e] and WANT dwords of `expected`;
// the path produces GOT dwords and dword k is compared with expected dword
// k % WANT. For a stochastic-rounding path a produced dword is one code (bit
// 16 set if the preserved part of the destination changed) and the expected
// dword holds the two bracket codes, low byte and next byte; it matches
// either. The random word advances once per entry with v_prng_b32 from
// fmix32(seed + lane * 0x85EBCA6B) | 1.
//
// Work split: 256 threads, one wave per SIMD. The block stages the three
// arrays from global memory into LDS once, 16 B per lane, then every wave
// walks the WHOLE table out of LDS, lane l taking entries l, l + 64, ..: each
// SIMD of the CU converts every operand. Nothing touches global memory between
// the staging and the record.
//
// Lane 0 of each wave writes one record of eight int32 (store_record8):
//   [0] placement word (hw_word; the SIMD is HW_ID[5:4])
//   [1] mismatched entries
//   [2] lowest bad entry (-1 if none)
//   [3] [4] the first mismatching produced dword of that entry and what was
//       expected there
//   [5] [6] checksum of every produced dword: xor, and xor of the dword times
//       (2 * position + 1)
//   [7] 0
// A stochastic-rounding path's checksum depends on which neighbour each entry
// took; it is the same in every healthy wave (same seed, same entries) and the
// host compares it by consensus, which names a SIMD that disagrees and cannot
// see a fault common to all.
// ---------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) short cvt_s2;
typedef __attribute__((ext_vector_type(2))) _Float16 cvt_h2;
typedef __attribute__((ext_vector_type(2))) __bf16 cvt_y2;
typedef __attribute__((ext_vector_type(32))) float f32x32;
typedef __attribute__((ext_vector_type(6))) unsigned u32x6;

constexpr int CVT_LDS_DWORDS = 32768;  // 128 KiB staging area
enum { CVT_FP8, CVT_BF8, CVT_FP6, CVT_BF6, CVT_FP4 };
enum { CVT_F32, CVT_F16, CVT_BF16 };

template <typename T> __device__ __forceinline__ unsigned cvt_bits(T v) {
  static_assert(sizeof(T) == 4, "one dword");
  return __builtin_bit_cast(unsigned, v);
}

template <int IN_, int WANT_, int GOT_, bool SR_ = false> struct CvtShape {
  static constexpr int IN = IN_, WANT = WANT_, GOT = GOT_;
  static constexpr bool SR = SR_;
};

// f32 / f16 / bf16 to two 8-bit codes, scaled; both word selects
template <int FMT, int W> struct CvtEnc8 : CvtShape<(W == CVT_F32 ? 2 : 1), 2, 2> {
  template <bool HI>
  static __device__ __forceinline__ unsigned one(const unsigned* in, float sc, cvt_s2 o) {
    if constexpr (W == CVT_F32) {
      const float a = __uint_as_float(in[0]), b = __uint_as_float(in[1]);
      if constexpr (FMT == CVT_FP8)
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_fp8_f32(o, a, b, sc, HI));
      else
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf8_f32(o, a, b, sc, HI));
    } else if constexpr (W == CVT_F16) {
      const cvt_h2 h = __builtin_bit_cast(cvt_h2, in[0]);
      if constexpr (FMT == CVT_FP8)
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_fp8_f16(o, h, sc, HI));
      else
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf8_f16(o, h, sc, HI));
    } else {
      const cvt_y2 y = __builtin_bit_cast(cvt_y2, in[0]);
      if constexpr (FMT == CVT_FP8)
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(o, y, sc, HI));
      else
        return cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf8_bf16(o, y, sc, HI));
    }
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const cvt_s2 o = __builtin_bit_cast(cvt_s2, old);
    got[0] = one<false>(in, sc, o);
    got[1] = one<true>(in, sc, o);
  }
};

// to two fp4 codes in the byte SEL names; all four byte selects
template <int W> struct CvtEnc4 : CvtShape<(W == CVT_F32 ? 2 : 1), 4, 4> {
  template <int SEL>
  static __device__ __forceinline__ unsigned one(const unsigned* in, float sc, unsigned old) {
    if constexpr (W == CVT_F32)
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, __uint_as_float(in[0]),
                                                      __uint_as_float(in[1]), sc, SEL);
    else if constexpr (W == CVT_F16)
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(old, __builtin_bit_cast(cvt_h2, in[0]), sc,
                                                      SEL);
    else
      return __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(old, __builtin_bit_cast(cvt_y2, in[0]), sc,
                                                       SEL);
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    got[0] = one<0>(in, sc, old);
    got[1] = one<1>(in, sc, old);
    got[2] = one<2>(in, sc, old);
    got[3] = one<3>(in, sc, old);
  }
};

// The 32-element converters write 6 or 32 VGPRs in several passes, and the
// compiler does not mark their destination early-clobber: in cvt_burn's fp6
// step it allocated `v_cvt_scalef32_2xpk16_fp6_f32 v[38:43], v[0:15],
// v[16:31], v38`, the scale in the first destination register, and every wave
// then produced the same wrong codes (BENCHMARKS.md "Conversion probe"). An
// operand that is still live after the instruction cannot share a register
// with its result, so each wrapper below keeps its operands alive past it.
template <typename T> __device__ __forceinline__ void cvt_keep(const T& v) {
  asm volatile("" : : "v"(v));
}

// 32 f32 to 32 six-bit codes in six dwords (the interleave: see above)
template <int FMT>
__device__ __forceinline__ u32x6 cvt_enc6(const unsigned* in, float sc) {
  f32x16 a, b;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    a[i] = __uint_as_float(in[2 * i]);
    b[i] = __uint_as_float(in[2 * i + 1]);
  }
  u32x6 p;
  if constexpr (FMT == CVT_FP6) p = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, sc);
  else p = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, sc);
  cvt_keep(a);
  cvt_keep(b);
  cvt_keep(sc);
  return p;
}
template <int FMT> __device__ __forceinline__ f32x32 cvt_dec6(u32x6 p, float sc) {
  f32x32 q;
  if constexpr (FMT == CVT_FP6) q = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(p, sc);
  else q = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(p, sc);
  cvt_keep(p);
  cvt_keep(sc);
  return q;
}
template <int FMT> struct CvtEnc6 : CvtShape<32, 6, 6> {
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const u32x6 p = cvt_enc6<FMT>(in, sc);
#pragma unroll
    for (int i = 0; i < 6; i++) got[i] = p[i];
  }
};
template <int FMT> struct CvtDec6 : CvtShape<6, 32, 32> {
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const u32x6 p = {in[0], in[1], in[2], in[3], in[4], in[5]};
    const f32x32 q = cvt_dec6<FMT>(p, sc);
#pragma unroll
    for (int i = 0; i < 32; i++) got[i] = __float_as_uint(q[i]);
  }
};

// four 8-bit codes to f32 (four dwords) or f16 / bf16 (two), scaled, through
// the packed form: both word selects
template <int FMT, int W> struct CvtDec8 : CvtShape<1, (W == CVT_F32 ? 4 : 2), (W == CVT_F32 ? 4 : 2)> {
  template <bool HI>
  static __device__ __forceinline__ void one(unsigned src, float sc, unsigned* got) {
    if constexpr (W == CVT_F32) {
      f32x2 d;
      if constexpr (FMT == CVT_FP8) d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(src, sc, HI);
      else d = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(src, sc, HI);
      got[2 * HI] = __float_as_uint(d[0]);
      got[2 * HI + 1] = __float_as_uint(d[1]);
    } else if constexpr (W == CVT_F16) {
      if constexpr (FMT == CVT_FP8)
        got[HI] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(src, sc, HI));
      else
        got[HI] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_f16_bf8(src, sc, HI));
    } else {
      if constexpr (FMT == CVT_FP8)
        got[HI] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(src, sc, HI));
      else
        got[HI] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(src, sc, HI));
    }
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    one<false>(in[0], sc, got);
    one<true>(in[0], sc, got);
  }
};

// four 8-bit codes to f32 through the byte-select form, scaled or not
template <int FMT, bool SCALED> struct CvtDecB8 : CvtShape<1, 4, 4> {
  template <int SEL> static __device__ __forceinline__ unsigned one(unsigned src, float sc) {
    if constexpr (SCALED) {
      if constexpr (FMT == CVT_FP8)
        return __float_as_uint(__builtin_amdgcn_cvt_scalef32_f32_fp8(src, sc, SEL));
      else
        return __float_as_uint(__builtin_amdgcn_cvt_scalef32_f32_bf8(src, sc, SEL));
    } else {
      if constexpr (FMT == CVT_FP8) return __float_as_uint(__builtin_amdgcn_cvt_f32_fp8(src, SEL));
      else return __float_as_uint(__builtin_amdgcn_cvt_f32_bf8(src, SEL));
    }
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    got[0] = one<0>(in[0], sc);
    got[1] = one<1>(in[0], sc);
    got[2] = one<2>(in[0], sc);
    got[3] = one<3>(in[0], sc);
  }
};

// eight fp4 codes to f32 (eight dwords) or f16 / bf16 (four): all byte selects
template <int W> struct CvtDec4 : CvtShape<1, (W == CVT_F32 ? 8 : 4), (W == CVT_F32 ? 8 : 4)> {
  template <int SEL>
  static __device__ __forceinline__ void one(unsigned src, float sc, unsigned* got) {
    if constexpr (W == CVT_F32) {
      const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(src, sc, SEL);
      got[2 * SEL] = __float_as_uint(d[0]);
      got[2 * SEL + 1] = __float_as_uint(d[1]);
    } else if constexpr (W == CVT_F16) {
      got[SEL] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(src, sc, SEL));
    } else {
      got[SEL] = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(src, sc, SEL));
    }
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    one<0>(in[0], sc, got);
    one<1>(in[0], sc, got);
    one<2>(in[0], sc, got);
    one<3>(in[0], sc, got);
  }
};

// the unscaled v_cvt_pk_{fp8,bf8}_f32 and v_cvt_pk_f32_{fp8,bf8}
template <int FMT> struct CvtEncU8 : CvtShape<2, 2, 2> {
  template <bool HI> static __device__ __forceinline__ unsigned one(float a, float b, int old) {
    if constexpr (FMT == CVT_FP8) return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, HI);
    else return (unsigned)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, HI);
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const float a = __uint_as_float(in[0]), b = __uint_as_float(in[1]);
    got[0] = one<false>(a, b, (int)old);
    got[1] = one<true>(a, b, (int)old);
  }
};
template <int FMT> struct CvtDecU8 : CvtShape<1, 4, 4> {
  template <bool HI> static __device__ __forceinline__ void one(unsigned src, unsigned* got) {
    f32x2 d;
    if constexpr (FMT == CVT_FP8) d = __builtin_amdgcn_cvt_pk_f32_fp8((int)src, HI);
    else d = __builtin_amdgcn_cvt_pk_f32_bf8((int)src, HI);
    got[2 * HI] = __float_as_uint(d[0]);
    got[2 * HI + 1] = __float_as_uint(d[1]);
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    one<false>(in[0], got);
    one<true>(in[0], got);
  }
};

// two f32 to a bf16 pair: the plain cast pair is v_cvt_pk_bf16_f32
struct CvtEncBf16 : CvtShape<2, 1, 1> {
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const cvt_y2 c = {(__bf16)__uint_as_float(in[0]), (__bf16)__uint_as_float(in[1])};
    got[0] = cvt_bits(c);
  }
};

// stochastic rounding. A produced dword is the code, with bit 16 set when the
// destination outside the written field no longer equals `old`.
__device__ __forceinline__ unsigned cvt_sr_field(unsigned d, unsigned old, int shift,
                                                 unsigned field) {
  return ((d >> shift) & field) | ((((d ^ old) & ~(field << shift)) != 0) ? 0x10000u : 0u);
}
template <int FMT, bool SCALED> struct CvtSr8 : CvtShape<1, 1, 4, true> {
  template <int SEL>
  static __device__ __forceinline__ unsigned one(float x, float sc, unsigned old, unsigned rnd) {
    unsigned d;
    if constexpr (SCALED) {
      if constexpr (FMT == CVT_FP8)
        d = (unsigned)__builtin_amdgcn_cvt_scalef32_sr_fp8_f32((int)old, x, rnd, sc, SEL);
      else
        d = (unsigned)__builtin_amdgcn_cvt_scalef32_sr_bf8_f32((int)old, x, rnd, sc, SEL);
    } else {
      if constexpr (FMT == CVT_FP8)
        d = (unsigned)__builtin_amdgcn_cvt_sr_fp8_f32(x, (int)rnd, (int)old, SEL);
      else
        d = (unsigned)__builtin_amdgcn_cvt_sr_bf8_f32(x, (int)rnd, (int)old, SEL);
    }
    return cvt_sr_field(d, old, 8 * SEL, 0xFFu);
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const float x = __uint_as_float(in[0]);
    got[0] = one<0>(x, sc, old, rnd);
    got[1] = one<1>(x, sc, old, rnd);
    got[2] = one<2>(x, sc, old, rnd);
    got[3] = one<3>(x, sc, old, rnd);
  }
};
struct CvtSr4 : CvtShape<2, 2, 8, true> {
  template <int SEL>
  static __device__ __forceinline__ void one(f32x2 x, float sc, unsigned old, unsigned rnd,
                                             unsigned* got) {
    // Issued as assembly: the compiler does not tie the `old` operand of
    // __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32 to the destination (it emits
    // the instruction into a fresh, uninitialised register), so through the
    // builtin the three bytes the instruction leaves alone are undefined. Here
    // the destination is a "+v" register that holds `old`. The byte select is
    // op_sel[2] (bit 0) and op_sel[3] (bit 1), as the builtin encodes it.
    unsigned d = old;
    if constexpr (SEL == 0)
      asm volatile("v_cvt_scalef32_sr_pk_fp4_f32 %0, %1, %2, %3"
                   : "+v"(d) : "v"(x), "v"(rnd), "v"(sc));
    else if constexpr (SEL == 1)
      asm volatile("v_cvt_scalef32_sr_pk_fp4_f32 %0, %1, %2, %3 op_sel:[0,0,1,0]"
                   : "+v"(d) : "v"(x), "v"(rnd), "v"(sc));
    else if constexpr (SEL == 2)
      asm volatile("v_cvt_scalef32_sr_pk_fp4_f32 %0, %1, %2, %3 op_sel:[0,0,0,1]"
                   : "+v"(d) : "v"(x), "v"(rnd), "v"(sc));
    else
      asm volatile("v_cvt_scalef32_sr_pk_fp4_f32 %0, %1, %2, %3 op_sel:[0,0,1,1]"
                   : "+v"(d) : "v"(x), "v"(rnd), "v"(sc));
    const unsigned byte = cvt_sr_field(d, old, 8 * SEL, 0xFFu);  // both codes and the flag
    got[2 * SEL] = byte & 0x1000Fu;
    got[2 * SEL + 1] = ((byte >> 4) & 0xFu) | (byte & 0x10000u);
  }
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    const f32x2 x = {__uint_as_float(in[0]), __uint_as_float(in[1])};
    one<0>(x, sc, old, rnd, got);
    one<1>(x, sc, old, rnd, got);
    one<2>(x, sc, old, rnd, got);
    one<3>(x, sc, old, rnd, got);
  }
};
template <int FMT> struct CvtSr6 : CvtShape<32, 32, 32, true> {
  static __device__ __forceinline__ void run(const unsigned* in, float sc, unsigned old,
                                             unsigned rnd, unsigned* got) {
    f32x32 v;
#pragma unroll
    for (int i = 0; i < 32; i++) v[i] = __uint_as_float(in[i]);
    u32x6 p;
    if constexpr (FMT == CVT_FP6) p = __builtin_amdgcn_cvt_scalef32_sr_pk32_fp6_f32(v, rnd, sc);
    else p = __builtin_amdgcn_cvt_scalef32_sr_pk32_bf6_f32(v, rnd, sc);
    cvt_keep(v);
    cvt_keep(rnd);
    cvt_keep(sc);
#pragma unroll
    for (int j = 0; j < 32; j++) {
      const int bit = 6 * j, word = bit >> 5, at = bit & 31;
      unsigned code = p[word] >> at;
      if (at + 6 > 32) code |= p[word + 1] << (32 - at);
      got[j] = code & 63u;
    }
  }
};

// index-aligned with CVT_PATH_NAMES
typedef std::tuple<
    CvtEnc8<CVT_FP8, CVT_F32>, CvtEnc8<CVT_BF8, CVT_F32>, CvtEnc8<CVT_FP8, CVT_F16>,
    CvtEnc8<CVT_BF8, CVT_F16>, CvtEnc8<CVT_FP8, CVT_BF16>, CvtEnc8<CVT_BF8, CVT_BF16>,
    CvtEnc4<CVT_F32>, CvtEnc4<CVT_F16>, CvtEnc4<CVT_BF16>, CvtEnc6<CVT_FP6>, CvtEnc6<CVT_BF6>,
    CvtDec8<CVT_FP8, CVT_F32>, CvtDec8<CVT_BF8, CVT_F32>, CvtDec8<CVT_FP8, CVT_F16>,
    CvtDec8<CVT_BF8, CVT_F16>, CvtDec8<CVT_FP8, CVT_BF16>, CvtDec8<CVT_BF8, CVT_BF16>,
    CvtDecB8<CVT_FP8, true>, CvtDecB8<CVT_BF8, true>, CvtDec4<CVT_F32>, CvtDec4<CVT_F16>,
    CvtDec4<CVT_BF16>, CvtDec6<CVT_FP6>, CvtDec6<CVT_BF6>, CvtEncU8<CVT_FP8>, CvtEncU8<CVT_BF8>,
    CvtDecU8<CVT_FP8>, CvtDecU8<CVT_BF8>, CvtDecB8<CVT_FP8, false>, CvtDecB8<CVT_BF8, false>,
    CvtEncBf16, CvtSr8<CVT_FP8, true>, CvtSr8<CVT_BF8, true>, CvtSr4, CvtSr6<CVT_FP6>,
    CvtSr6<CVT_BF6>, CvtSr8<CVT_FP8, false>, CvtSr8<CVT_BF8, false>>
    CvtPathTypes;
constexpr int CVT_PATHS = std::tuple_size<CvtPathTypes>::value;
static const char* const CVT_PATH_NAMES[CVT_PATHS] = {
    "enc_fp8_f32",  "enc_bf8_f32",  "enc_fp8_f16",   "enc_bf8_f16",   "enc_fp8_bf16",
    "enc_bf8_bf16", "enc_fp4_f32",  "enc_fp4_f16",   "enc_fp4_bf16",  "enc_fp6_f32",
    "enc_bf6_f32",  "dec_f32_fp8",  "dec_f32_bf8",   "dec_f16_fp8",   "dec_f16_bf8",
    "dec_bf16_fp8", "dec_bf16_bf8", "decb_f32_fp8",  "decb_f32_bf8",  "dec_f32_fp4",
    "dec_f16_fp4",  "dec_bf16_fp4", "dec_f32_fp6",   "dec_f32_bf6",   "encu_fp8_f32",
    "encu_bf8_f32", "decu_f32_fp8", "decu_f32_bf8",  "decub_f32_fp8", "decub_f32_bf8",
    "enc_bf16_f32", "sr_fp8_f32",   "sr_bf8_f32",    "sr_fp4_f32",    "sr_fp6_f32",
    "sr_bf6_f32",   "sru_fp8_f32",  "sru_bf8_f32"};

// where the scales and the expected dwords start in the staging area: each
// array begins on a 16 B boundary
__host__ __device__ constexpr int cvt_round4(int n) { return (n + 3) & ~3; }

// n dwords from 16 B aligned global memory into 16 B aligned LDS, 16 B per lane
__device__ __forceinline__ void cvt_stage(unsigned* __restrict__ dst,
                                          const unsigned* __restrict__ src, int n) {
  const uint4* src4 = reinterpret_cast<const uint4*>(src);
  uint4* dst4 = reinterpret_cast<uint4*>(dst);
  for (int i = threadIdx.x; i < (n >> 2); i += blockDim.x) dst4[i] = src4[i];
  for (int i = (n & ~3) + threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

template <typename P>
__global__ void __launch_bounds__(256)
cvt_sweep_kernel(const unsigned* __restrict__ inputs, const unsigned* __restrict__ scales,
                 const unsigned* __restrict__ expected, int4* __restrict__ records, int entries,
                 unsigned seed) {
  __shared__ uint4 staged[CVT_LDS_DWORDS / 4];
  unsigned* lds = reinterpret_cast<unsigned*>(staged);
  const int off_scale = cvt_round4(entries * P::IN);
  const int off_want = off_scale + cvt_round4(entries);
  cvt_stage(lds, inputs, entries * P::IN);
  cvt_stage(lds + off_scale, scales, entries);
  cvt_stage(lds + off_want, expected, entries * P::WANT);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned place = hw_word();
  unsigned rnd = fmix32(seed + (unsigned)lane * 0x85EBCA6Bu) | 1u;
  unsigned mismatched = 0, first = 0x7FFFFFFFu, first_got = 0, first_want = 0;
  unsigned sum_lo = 0, sum_hi = 0;
  for (int e = lane; e < entries; e += 64) {
    unsigned in[P::IN], want[P::WANT], got[P::GOT];
#pragma unroll
    for (int j = 0; j < P::IN; j++) in[j] = lds[e * P::IN + j];
#pragma unroll
    for (int j = 0; j < P::WANT; j++) want[j] = lds[off_want + e * P::WANT + j];
    const float sc = __uint_as_float(lds[off_scale + e]);
    const unsigned old = fmix32((unsigned)e * 0x9E3779B1u + 0x85EBCA6Bu);
    if constexpr (P::SR) rnd = __builtin_amdgcn_prng_b32(rnd);
    P::run(in, sc, old, rnd, got);
    bool bad = false;
    unsigned bad_got = 0, bad_want = 0;
#pragma unroll
    for (int k = P::GOT - 1; k >= 0; k--) {  // downwards: the first bad dword is kept
      const unsigned w = want[k % P::WANT];
      bool same = got[k] == w;
      if constexpr (P::SR) same = got[k] == (w & 0xFFu) || got[k] == ((w >> 8) & 0xFFu);
      if (!same) {
        bad = true;
        bad_got = got[k];
        bad_want = w;
      }
      sum_lo ^= got[k];
      sum_hi ^= got[k] * (2u * (unsigned)(e * P::GOT + k) + 1u);
    }
    if (bad) {
      mismatched++;
      if (first == 0x7FFFFFFFu) {  // a lane's entries ascend
        first = (unsigned)e;
        first_got = bad_got;
        first_want = bad_want;
      }
    }
  }
  mismatched = wave_add(mismatched);
  const unsigned lowest = wave_min(first);
  const int owner = (int)(lowest & 63u);  // entry e belongs to lane e % 64
  first_got = (unsigned)__shfl((int)first_got, owner);
  first_want = (unsigned)__shfl((int)first_want, owner);
  sum_lo = wave_xor(sum_lo);
  sum_hi = wave_xor(sum_hi);
  if (lane == 0)
    store_record8(records, wave, (int)place, (int)mismatched,
                  lowest == 0x7FFFFFFFu ? -1 : (int)lowest, (int)first_got, (int)first_want,
                  (int)sum_lo, (int)sum_hi, 0);
}

// a 1-D contiguous tensor of `dtype` on `device` whose storage starts on 16 B
static void cvt_check_table(const torch::Tensor& t, const char* name, c10::ScalarType dtype,
                            torch::Device device) {
  TORCH_CHECK(t.is_cuda() && t.device() == device, name, " must be on the GPU of `inputs`");
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ", c10::toString(dtype));
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous(), name, " must be 1-D and contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must start on a 16 B boundary");
}

// inputs: int32 [entries * IN], scales: float32 [entries], expected: int32
// [entries * WANT] for the path's IN and WANT (ops/cvt_probe.py builds them).
// Returns (records [blocks*4, 8] int32, elapsed_ms of the one launch).
std::tuple<torch::Tensor, double> cvt_sweep(const std::string& path, torch::Tensor inputs,
                                            torch::Tensor scales, torch::Tensor expected,
                                            long blocks, long seed) {
  int id = -1;
  for (int p = 0; p < CVT_PATHS; p++)
    if (path == CVT_PATH_NAMES[p]) id = p;
  TORCH_CHECK(id >= 0, "unknown conversion path ", path);
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  TORCH_CHECK(inputs.is_cuda() && inputs.get_device() == dev,
              "inputs must be on the current GPU");
  cvt_check_table(inputs, "inputs", torch::kInt32, inputs.device());
  cvt_check_table(scales, "scales", torch::kFloat32, inputs.device());
  cvt_check_table(expected, "expected", torch::kInt32, inputs.device());
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 16), "blocks must be in [1, 2^16]");
  const long entries = scales.numel();
  TORCH_CHECK(entries >= 1 && entries <= CVT_LDS_DWORDS, "the table needs 1 to ", CVT_LDS_DWORDS,
              " entries");
  auto records = zero_records(blocks * 4, 8, inputs.device());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  double ms = 0;
  dispatch_int<CVT_PATHS>(id, [&](auto id_c) {
    typedef std::tuple_element_t<decltype(id_c)::value, CvtPathTypes> P;
    TORCH_CHECK(inputs.numel() == entries * P::IN && expected.numel() == entries * P::WANT, path,
                ": ", entries, " scales need ", entries * P::IN, " input and ", entries * P::WANT,
                " expected dwords");
    const long need = cvt_round4(entries * P::IN) + cvt_round4(entries) + entries * P::WANT;
    TORCH_CHECK(need <= CVT_LDS_DWORDS, path, ": the table takes ", need,
                " dwords, the LDS staging area holds ", CVT_LDS_DWORDS);
    ms = timed_ms(stream, [&]() {
      hipLaunchKernelGGL((cvt_sweep_kernel<P>), dim3(blocks), dim3(256), 0, stream,
                         reinterpret_cast<const unsigned*>(inputs.data_ptr<int>()),
                         reinterpret_cast<const unsigned*>(scales.data_ptr<float>()),
                         reinterpret_cast<const unsigned*>(expected.data_ptr<int>()),
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (int)entries,
                         (unsigned)seed);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// Conversion burn: the VALU burn's contract (a u32 state per lane seeded from
// (seed, section, lane) only, `chain` dependent steps per round, a bitwise
// compare against expected[lane] each round, the same record and the same
// register-only inject) with a step made of converters. A step
//   1. carves wide values out of the state: a hash of the state gives sign
//      and 23 mantissa bits, and the exponent is e + k with e inside the
//      format's normal range below its top binade (so rounding up stays within
//      max normal) and k in [-8, 7] the encode scale, also from the state
//   2. encodes them with the scale 2^k
//   3. decodes the codes with a second scale 2^k2
//   4. folds the code bits and the decoded floats' bits into the state with a
//      multiply-xor
// Sections: fp8, bf8 (v_cvt_scalef32_pk_{fp8,bf8}_f32 and pk_f32_{fp8,bf8}),
// fp4 (pk_fp4_f32, pk_f32_fp4), fp6 (32 values per lane through 2xpk16_fp6_f32
// and pk32_f32_fp6), bf16 (v_cvt_pk_bf16_f32; a bf16's f32 value is its bits
// shifted, so the decode is no instruction). ops.cvt_burn_expected reproduces
// every section bit for bit from the sweep's encode and decode functions. The
// hot loop has no memory traffic. Record: as valu_burn.
// ---------------------------------------------------------------------------
enum { CVTB_FP8, CVTB_BF8, CVTB_FP6, CVTB_FP4, CVTB_BF16, CVTB_SECTIONS };
static const char* const CVTB_NAMES[CVTB_SECTIONS] = {"fp8", "bf8", "fp6", "fp4", "bf16"};

// sign and mantissa from h[31] and h[22:0]; exponent EMIN + (h[30:23] * NEXP >> 8) + k
template <int EMIN, int NEXP> __device__ __forceinline__ float cvt_carve(unsigned h, int k) {
  const int e = EMIN + (int)((((h >> 23) & 0xFFu) * NEXP) >> 8);
  return __uint_as_float((h & 0x807FFFFFu) | ((unsigned)(127 + e + k) << 23));
}
__device__ __forceinline__ unsigned cvt_hash(unsigned x, unsigned mul) {
  x *= mul;
  return x ^ (x >> 15);
}
__device__ __forceinline__ float cvt_pow2(int k) {
  return __uint_as_float((unsigned)(127 + k) << 23);
}

template <int SEC> struct CvtBurnStep {
  static __device__ __forceinline__ unsigned step(unsigned s) {
    const int k = (int)((s >> 3) & 15u) - 8, k2 = (int)((s >> 9) & 15u) - 8;
    const float sc = cvt_pow2(k), sc2 = cvt_pow2(k2);
    const unsigned next = s * 0x9E3779B1u + 0x7F4A7C15u;
    const unsigned h0 = cvt_hash(s, 0x85EBCA6Bu), h1 = cvt_hash(s ^ 0xC2B2AE35u, 0x27D4EB2Fu);
    if constexpr (SEC == CVTB_FP8) {
      const cvt_s2 zero = {0, 0};
      const unsigned w = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_fp8_f32(
          zero, cvt_carve<-6, 14>(h0, k), cvt_carve<-6, 14>(h1, k), sc, false));
      const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, sc2, false);
      return next ^ w ^ rotl32(__float_as_uint(d[0]), 7) ^ rotl32(__float_as_uint(d[1]), 19);
    } else if constexpr (SEC == CVTB_BF8) {
      const cvt_s2 zero = {0, 0};
      const unsigned w = cvt_bits(__builtin_amdgcn_cvt_scalef32_pk_bf8_f32(
          zero, cvt_carve<-14, 29>(h0, k), cvt_carve<-14, 29>(h1, k), sc, false));
      const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(w, sc2, false);
      return next ^ w ^ rotl32(__float_as_uint(d[0]), 7) ^ rotl32(__float_as_uint(d[1]), 19);
    } else if constexpr (SEC == CVTB_FP4) {
      const unsigned w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(
          0u, cvt_carve<0, 2>(h0, k), cvt_carve<0, 2>(h1, k), sc, 0);
      const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, sc2, 0);
      return next ^ w ^ rotl32(__float_as_uint(d[0]), 7) ^ rotl32(__float_as_uint(d[1]), 19);
    } else if constexpr (SEC == CVTB_FP6) {
      unsigned in[32];
#pragma unroll
      for (int j = 0; j < 32; j++)
        in[j] = __float_as_uint(
            cvt_carve<0, 2>(cvt_hash(s ^ ((unsigned)j * 0x85EBCA6Bu), 0x9E3779B1u), k));
      const u32x6 p = cvt_enc6<CVT_FP6>(in, sc);
      const f32x32 q = cvt_dec6<CVT_FP6>(p, sc2);
      unsigned x = next;
#pragma unroll
      for (int i = 0; i < 6; i++) x ^= rotl32(p[i], 5 * i + 1);
#pragma unroll
      for (int j = 0; j < 32; j++) x ^= rotl32(__float_as_uint(q[j]), j % 31 + 1);
      return x;
    } else {
      const cvt_y2 c = {(__bf16)cvt_carve<-100, 200>(h0, k), (__bf16)cvt_carve<-100, 200>(h1, k)};
      const unsigned w = cvt_bits(c);
      return next ^ w ^ rotl32(w << 16, 7) ^ rotl32(w & 0xFFFF0000u, 19);
    }
  }
};

template <int SEC>
__global__ void __launch_bounds__(256)
cvt_burn_kernel(const unsigned* __restrict__ expected, int4* __restrict__ records, unsigned seed,
                int chain, int rounds, int inject_wave, int inject_round, int inject_lane,
                int inject_bit) {
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned place = hw_word();
  const unsigned seeded =
      fmix32(seed + (unsigned)(SEC + 16) * 0x9E3779B9u + (unsigned)lane * 0x85EBCA6Bu);
  const unsigned want = expected[lane];
  const unsigned flip = (wave == inject_wave && lane == inject_lane) ? 1u << (inject_bit & 31) : 0u;
  int mismatched = 0, first_round = -1, first_lane = -1;
  unsigned checksum = 0;
  for (int round = 0; round < rounds; round++) {
    unsigned s = seeded;
    // opaque to the optimiser: every round really recomputes its chain
    asm volatile("" : "+v"(s));
    for (int c = 0; c < chain; c++) s = CvtBurnStep<SEC>::step(s);
    if (round == inject_round) s ^= flip;
    checksum ^= s;
    const unsigned long long bad = __ballot(s != want);  // wave-uniform
    if (bad) {
      mismatched += __popcll(bad);
      if (first_round < 0) {
        first_round = round;
        first_lane = __ffsll((long long)bad) - 1;
      }
    }
  }
  checksum = wave_xor(checksum);
  if (lane == 0)
    store_record8(records, wave, (int)place, mismatched, first_round, first_lane, (int)checksum, 0,
                  0, 0);
}

// expected: 64 int32 on the current device, the state every lane must reach
// after `chain` steps (ops.cvt_burn_expected). One untimed warm-up launch,
// then one timed launch (warm_then_timed_ms).
// Returns (records [waves,8] int32, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, double> cvt_burn(const std::string& section, torch::Tensor expected,
                                           long seed, long blocks, long chain, long rounds,
                                           long inject_wave, long inject_round, long inject_lane,
                                           long inject_bit) {
  int sec = -1;
  for (int s = 0; s < CVTB_SECTIONS; s++)
    if (section == CVTB_NAMES[s]) sec = s;
  TORCH_CHECK(sec >= 0, "section must be one of fp8, bf8, fp6, fp4, bf16; got ", section);
  TORCH_CHECK(blocks >= 1 && blocks <= (1L << 20), "blocks must be in [1, 2^20]");
  TORCH_CHECK(chain >= 1 && rounds >= 1, "chain and rounds must be >= 1");
  // every round ends in the same state: the xor checksum of an even number
  // of rounds is zero whatever the hardware computed
  TORCH_CHECK(rounds % 2 == 1, "rounds must be odd (the xor checksum cancels over an even number)");
  TORCH_CHECK(chain <= (1L << 22) && rounds <= (1L << 22) && chain * rounds <= (1L << 22),
              "chain*rounds must be <= 2^22");
  TORCH_CHECK(inject_wave >= -1 && inject_wave < blocks * 4 && inject_round >= -1 &&
                  inject_round < rounds && inject_lane >= -1 && inject_lane < 64 &&
                  inject_bit >= -1 && inject_bit < 32,
              "inject_wave/inject_round/inject_lane/inject_bit out of range");
  TORCH_CHECK(inject_wave < 0 || (inject_round >= 0 && inject_lane >= 0 && inject_bit >= 0),
              "an injection needs inject_round, inject_lane and inject_bit");
  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  TORCH_CHECK(expected.is_cuda() && expected.get_device() == dev,
              "expected must be on the current GPU");
  TORCH_CHECK(expected.dtype() == torch::kInt32 && expected.numel() == 64 &&
                  expected.is_contiguous(),
              "expected must hold 64 contiguous int32 values (one state per lane)");
  auto records = zero_records(blocks * 4, 8);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<CVTB_SECTIONS>(sec, [&](auto sec_c) {
      hipLaunchKernelGGL((cvt_burn_kernel<decltype(sec_c)::value>), dim3(blocks), dim3(256), 0,
                         stream, reinterpret_cast<const unsigned*>(expected.data_ptr<int>()),
                         reinterpret_cast<int4*>(records.data_ptr<int>()), (unsigned)seed,
                         (int)chain, (int)rounds, (int)inject_wave, (int)inject_round,
                         (int)inject_lane, (int)inject_bit);
    });
  });
  return std::make_tuple(records, ms);
}

// ---------------------------------------------------------------------------
// GEMM probe: every probe above exercises one unit at a time. A tenant's GEMM
// keeps direct-to-LDS loads in flight, reads LDS into fragments and issues
// MFMAs back to back, in the same cycles on every CU. gemm_pipe_kernel is that
// combined load as a real tiled GEMM whose result is exact by construction
// (ops/gemm_probe.py) and compared bitwise in registers; lds_tr_read_kernel
// underneath it checks the gfx950 LDS transpose reads as plain data movement.
//
// --- lds_tr_read: the transpose-read map ---
// ds_read_b64_tr_b16 / _b8 / _b4 and ds_read_b96_tr_b6, from the LLVM AMDGPU
// description of llvm.amdgcn.ds.read.tr{16,8,4}.b64 / tr6.b96 and ck_tile's
// LaneGroupTransposeTraits and DefaultTranspose::Quad16 / Quad8 encodings: the
// wave is four groups of 16 lanes. A group's lanes together address a block of
// R rows of 16 elements of WIDTH bits, R = 64 / WIDTH (16 for the 6-bit form:
// 96 bits per lane), each lane 64 (96) consecutive bits of one row, row-major
// over the lanes: with P = 16 / R lanes per row, lane i of the group supplies
// elements (16 / P) (i % P) onwards of row i / P. Lane i of the group receives
// column i of that block, row 0 in the lowest bits. Rows need not be adjacent
// in LDS: every lane gives its own byte address. ck_tile states this for 16 and
// 8 bits; for 4 and 6 bits it is the same rule with one lane per row.
// Alignment: the b64 forms need an 8-byte address like ds_read_b64; the b96
// form is held to 16 bytes like ds_read_b96 in aligned mode (stricter than the
// hardware may need, so safe). One wave copies the image into LDS, each lane
// issues one read at addrs[lane] and stores its 2 (3) result words. The wrapper
// refuses an address outside the image or misaligned, so a bad argument cannot
// become a bad access.
//
// --- gemm_pipe: C = A.B, fp32 accumulate ---
// FMT bf16 (v_mfma_f32_16x16x32_bf16) or fp8 e4m3 (v_mfma_f32_16x16x32_fp8_fp8).
// A [M,K] K-contiguous. BLAYOUT kn: B [K,N] N-contiguous, fragments through the
// transpose reads (tr_b16 / tr_b8); nk: B [N,K] K-contiguous, fragments through
// ds_read_b128. One workgroup of 256 threads per 128x128 tile of C, waves 2x2,
// 64x64 per wave as 4x4 MFMA tiles (64 accumulator registers) held for the
// whole K loop. A K step is 128 bytes of K per row: 64 bf16 or 128 fp8.
//
// Data flow per K step: 16 KiB of A and 16 KiB of B go from global memory to
// LDS with global_load_lds_dwordx4 (lane l's 16 bytes land at M0 + 16 l, as the
// memory-path probe established), 1 KiB per instruction, four A and four B
// instructions per wave. Two LDS stages of 32 KiB (64 KiB: two workgroups per
// CU). Step k+1's eight loads are issued before step k is waited for with
// s_waitcnt vmcnt(8), so they are in flight while step k's MFMAs issue; the
// last step waits vmcnt(0). Barrier 1 (before the issue): every wave has read
// stage (k+1)&1 for the last time. Barrier 2 (after the wait): every wave's
// part of step k has landed. A step's fragment reads are issued as two halves
// (K/2 each); the first half's MFMAs wait for lgkmcnt(8) (kn: 12), the reads
// of the second half still in flight, the second half's for lgkmcnt(0). No
// wave waits for another workgroup; every loop bound is a launch argument.
//
// LDS map of a stage: A tile at 0, B tile at 16 KiB. Rows are 128 bytes = 8
// chunks of 16 bytes (kn bf16: a B row is one k, 256 bytes = 16 chunks). The
// direct load fixes where a lane's 16 bytes land, so the swizzle is on the
// source side: the lane that lands in (row r, slot s) fetches global chunk
// s ^ key(r) (kn bf16: s ^ 2 key), and a reader wanting chunk q of row r reads
// slot q ^ key(r). Keys (3 bits):
//   A, B nk  ds_read_b128, 16 lanes = 16 rows, one chunk:  key = (r>>1) & 7
//   B kn fp8 tr_b8, 32 lanes = rows k..k+7, k+16..k+23:     key = (k>>1)&3 | (k>>4&1)<<2
//   B kn bf16 tr_b16, 32 lanes = rows k..k+3, k+8..k+11,
//            two chunks each:                               key = k&3 | (k>>3&1)<<2
// A row of 128 bytes covers half of the 64 banks, so rows r and r+1 never
// collide and rows r, r+2 do: each key is a bijection on the rows of one
// access that share a half. Remaining conflict degree: none by construction,
// under the assumption that one LDS pass serves 16 consecutive lanes of a
// b128 read and 32 of a b64 read; not measured with counters.
// fp8: a lane's 16 bytes of A (and of B nk) are 16 consecutive k, used as two
// MFMAs (low and high 8 bytes); the transposed B reads follow that k order.
// Any consistent K order gives the same bits, the sums being exact.
//
// Verification in registers, the same code in this kernel, mx_gemm_pipe_kernel
// and mx6_gemm_pipe_kernel (GP_ZERO_ACC, gp_inject, gp_compare_round,
// gp_store_c, gp_store_record): per round the accumulators are zeroed (opaque
// to the optimiser), the K loop runs, every element is compared bitwise with
// expected[128,128] and xor-ed into a checksum. Lane 0 of each wave writes
// (store_record8): [0] placement word, [1] mismatched elements, [2] first bad
// round (-1), [3] index of the first bad element of that round in the wave's
// 64x64 block, row-major (-1), [4] xor of all accumulator bits, [5..7] 0.
// store_c: the last round's tile also goes to C[M,N]. inject_block /
// inject_round: lane 0 of wave 0 of that workgroup flips the low mantissa bit
// of its first accumulator element before the compare: register arithmetic only.
// The addresses of the compare and of the store are worked out after the K
// loop from a lane index made opaque there, so that none is held over it.
//
// Checked in the gfx950 disassembly: per K step and wave eight
// global_load_lds_dwordx4, then s_waitcnt vmcnt(8) and no other vmcnt wait
// inside the K loop but the last step's vmcnt(0); 16 ds_read_b128 (nk) or 8
// ds_read_b128 and 16 ds_read_b64_tr_b16 / _tr_b8 (kn), s_waitcnt lgkmcnt(8 / 12)
// before the first 16 (fp8: 32) MFMAs and lgkmcnt(0) before the rest; two
// s_barrier per step and one per round. Build: no scratch, 64 KiB of LDS,
// accumulators in architectural VGPRs (register counts in BENCHMARKS.md "GEMM
// probe").
// ---------------------------------------------------------------------------
#define GP_LDS_AS __attribute__((address_space(3)))
#define GP_GLOBAL_AS __attribute__((address_space(1)))
typedef short gp_s4 __attribute__((ext_vector_type(4)));
typedef int gp_i2 __attribute__((ext_vector_type(2)));
typedef int gp_i3 __attribute__((ext_vector_type(3)));
typedef int gp_i4 __attribute__((ext_vector_type(4)));
constexpr int TR_IMAGE_MAX_WORDS = 4096;  // 16 KiB

template <int WIDTH>
__global__ void __launch_bounds__(64)
lds_tr_read_kernel(const int* __restrict__ image, int words, const int* __restrict__ addrs,
                   int* __restrict__ regs) {
  __shared__ __attribute__((aligned(16))) int img[TR_IMAGE_MAX_WORDS];
  const int lane = threadIdx.x;
  for (int i = lane; i < words; i += 64) img[i] = image[i];
  __syncthreads();
  GP_LDS_AS char* at = (GP_LDS_AS char*)img + addrs[lane];
  if constexpr (WIDTH == 6) {
    const gp_i3 v = __builtin_amdgcn_ds_read_tr6_b96_v3i32((GP_LDS_AS gp_i3*)at);
    regs[3 * lane] = v[0];
    regs[3 * lane + 1] = v[1];
    regs[3 * lane + 2] = v[2];
  } else {
    gp_i2 v;
    if constexpr (WIDTH == 16) {
      const gp_s4 h = __builtin_amdgcn_ds_read_tr16_b64_v4i16((GP_LDS_AS gp_s4*)at);
      v = __builtin_bit_cast(gp_i2, h);
    } else if constexpr (WIDTH == 8) {
      v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((GP_LDS_AS gp_i2*)at);
    } else {
      v = __builtin_amdgcn_ds_read_tr4_b64_v2i32((GP_LDS_AS gp_i2*)at);
    }
    regs[2 * lane] = v[0];
    regs[2 * lane + 1] = v[1];
  }
}

enum { GP_BF16 = 0, GP_FP8 = 1 };
enum { GP_KN = 0, GP_NK = 1 };
constexpr int GP_TILE = 128;          // C tile edge per workgroup
constexpr int GP_STEP_BYTES = 128;    // bytes of K per row and step
constexpr int GP_TILE_BYTES = 16384;  // one operand tile of one step
constexpr int GP_STAGE_BYTES = 2 * GP_TILE_BYTES;
constexpr int GP_STAGES = 2;

// swizzle keys (see the LDS map above)
__device__ __forceinline__ int gp_key_b128(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int gp_key_tr8(int k) { return ((k >> 1) & 3) | (((k >> 4) & 1) << 2); }
__device__ __forceinline__ int gp_key_tr16(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }

// the eight direct-to-LDS loads of one wave for one K step
__device__ __forceinline__ void gp_issue(const char* a_src, const char* b_src,
                                         const unsigned (&aoff)[4], const unsigned (&boff)[4],
                                         GP_LDS_AS char* stage, int wave) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    GP_LDS_AS char* to = stage + (wave * 4 + i) * 1024;  // wave-uniform: goes to M0
    __builtin_amdgcn_global_load_lds((GP_GLOBAL_AS const unsigned*)(a_src + aoff[i]),
                                     (GP_LDS_AS unsigned*)to, 16, 0, 0);
    __builtin_amdgcn_global_load_lds((GP_GLOBAL_AS const unsigned*)(b_src + boff[i]),
                                     (GP_LDS_AS unsigned*)(to + GP_TILE_BYTES), 16, 0, 0);
  }
}

// LDS reads of the GEMM as inline assembly: through the builtins or plain
// loads the compiler cannot tell the LDS a direct load writes from the LDS a
// read touches and puts s_waitcnt vmcnt(0) before the first read of a step,
// which drains the loads of step k+1. The asm reads are waited for with explicit
// lgkmcnt counts that name the registers, so no use can move above the wait.
// The offset is an immediate: the 24 (nk: 16) reads of a step share six (four)
// address registers.
#define GP_READ(INSN, DST, AT, OFF) \
  asm volatile(INSN " %0, %1 offset:" #OFF : "=v"(DST) : "v"(AT) : "memory")
template <int BL> struct GpFrags {
  gp_i4 a[4];
  gp_i4 b[4];            // nk: one ds_read_b128 per tile
  gp_i2 lo[4], hi[4];    // kn: two transpose reads per tile
};
// HS: which half of the K step. a_at, b_at: LDS byte addresses in the stage,
// a_at of tile 0 of this half; b_at nk: [0] of tile 0 of this half, kn: of each
// tile's first read of half 0.
template <int FMT, int BL, int HS>
__device__ __forceinline__ void gp_read_half(GpFrags<BL>& f, unsigned a_at,
                                             const unsigned (&b_at)[4]) {
  GP_READ("ds_read_b128", f.a[0], a_at, 0);
  GP_READ("ds_read_b128", f.a[1], a_at, 2048);
  GP_READ("ds_read_b128", f.a[2], a_at, 4096);
  GP_READ("ds_read_b128", f.a[3], a_at, 6144);
  if constexpr (BL == GP_NK) {
    GP_READ("ds_read_b128", f.b[0], b_at[0], 16384);
    GP_READ("ds_read_b128", f.b[1], b_at[0], 18432);
    GP_READ("ds_read_b128", f.b[2], b_at[0], 20480);
    GP_READ("ds_read_b128", f.b[3], b_at[0], 22528);
  } else {
    // half 1 is 32 (fp8: 64) k rows = 8192 bytes on; hi is 4 (8) rows = 1024 on
#define GP_READ_TR(INSN)                                    \
  _Pragma("unroll") for (int t = 0; t < 4; t++) {           \
    if constexpr (HS == 0) {                                \
      GP_READ(INSN, f.lo[t], b_at[t], 16384);               \
      GP_READ(INSN, f.hi[t], b_at[t], 17408);               \
    } else {                                                \
      GP_READ(INSN, f.lo[t], b_at[t], 24576);               \
      GP_READ(INSN, f.hi[t], b_at[t], 25600);               \
    }                                                       \
  }
    if constexpr (FMT == GP_BF16) {
      GP_READ_TR("ds_read_b64_tr_b16")
    } else {
      GP_READ_TR("ds_read_b64_tr_b8")
    }
#undef GP_READ_TR
  }
}
#undef GP_READ
// wait until this half's reads have returned; OTHERS: the reads of the other
// half (8 nk, 12 kn) were issued after them and may stay in flight
template <int BL, bool OTHERS>
__device__ __forceinline__ void gp_wait_half(GpFrags<BL>& f) {
  if constexpr (BL == GP_NK) {
#define GP_WAIT_NK(CNT)                                                                     \
  asm volatile("s_waitcnt lgkmcnt(" CNT ")"                                                 \
               : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]),      \
                 "+v"(f.b[1]), "+v"(f.b[2]), "+v"(f.b[3])::"memory")
    if constexpr (OTHERS) GP_WAIT_NK("8");
    else GP_WAIT_NK("0");
#undef GP_WAIT_NK
  } else {
#define GP_WAIT_KN(CNT)                                                                     \
  asm volatile("s_waitcnt lgkmcnt(" CNT ")"                                                 \
               : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.lo[0]),     \
                 "+v"(f.lo[1]), "+v"(f.lo[2]), "+v"(f.lo[3]), "+v"(f.hi[0]), "+v"(f.hi[1]), \
                 "+v"(f.hi[2]), "+v"(f.hi[3])::"memory")
    if constexpr (OTHERS) GP_WAIT_KN("12");
    else GP_WAIT_KN("0");
#undef GP_WAIT_KN
  }
}
template <int FMT, int BL>
__device__ __forceinline__ void gp_mma_half(const GpFrags<BL>& f, f32x4 (&acc)[4][4]) {
  typedef long gp_l2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      gp_i4 b;
      if constexpr (BL == GP_NK) b = f.b[j];
      else b = (gp_i4){f.lo[j][0], f.lo[j][1], f.hi[j][0], f.hi[j][1]};
      if constexpr (FMT == GP_BF16) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(frag8, f.a[i]), __builtin_bit_cast(frag8, b), acc[i][j], 0, 0, 0);
      } else {
        const gp_l2 al = __builtin_bit_cast(gp_l2, f.a[i]), bl = __builtin_bit_cast(gp_l2, b);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(al[0], bl[0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(al[1], bl[1], acc[i][j], 0, 0, 0);
      }
    }
}

// LDS byte offsets of this lane's fragment reads inside a stage (the B tile's
// 16 KiB are in the instruction's offset), where gemm_pipe_kernel and
// mx_gemm_pipe_kernel read alike: A and B nk through ds_read_b128, B kn fp8
// through tr_b8 (a kn B of another width fills b_at itself). The keys do not
// depend on the tile (A, B nk) or on the half and the read (B kn), so the
// other reads are a constant number of bytes on; half 1 (chunk g + 4) of A
// and B nk is chunk q ^ 4.
template <int BL>
__device__ __forceinline__ void gp_frag_addrs(unsigned (&a_at)[2], unsigned (&b_at)[4], int wm,
                                              int wn, int i16, int g) {
  const int ra = wm * 64 + i16;
  a_at[0] = ra * 128 + ((g ^ gp_key_b128(ra)) << 4);
  a_at[1] = a_at[0] ^ 64;
  if constexpr (BL == GP_NK) {
    const int rb = wn * 64 + i16;
    b_at[0] = rb * 128 + ((g ^ gp_key_b128(rb)) << 4);
    b_at[1] = b_at[0] ^ 64;
    b_at[2] = b_at[3] = 0;
  } else {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int nb = wn * 64 + t * 16;
      const int k = g * 16 + (i16 >> 1);
      b_at[t] = k * 128 + (((nb >> 4) ^ gp_key_tr8(k)) << 4) + (i16 & 1) * 8;
    }
  }
}

// --- around the K loop: what gemm_pipe_kernel, mx_gemm_pipe_kernel and
// mx6_gemm_pipe_kernel do with the wave's 4x4 accumulator tiles (see
// "Verification in registers" above) ---
struct GpVerdict {  // fields [1..4] of the wave's record
  int mismatched = 0, first_round = -1;
  unsigned first_index = 0xFFFFFFFFu, checksum = 0;
};

// Zeroes the accumulators, opaque to the optimiser: every round really
// recomputes its tile. A macro: the same statements inlined from a function
// cost mx6_gemm_pipe_kernel<8, 4, nk> one VGPR more (184), outside the K loop.
#define GP_ZERO_ACC(ACC)                                \
  _Pragma("unroll") for (int i = 0; i < 4; i++) {       \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {     \
      ACC[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};          \
      asm volatile("" : "+v"(ACC[i][j]));               \
    }                                                   \
  }

// the injected fault: the low mantissa bit of the lane's first element
__device__ __forceinline__ void gp_inject(f32x4 (&acc)[4][4]) {
  acc[0][0][0] = __uint_as_float(__float_as_uint(acc[0][0][0]) ^ 1u);
}

// One round's compare. expected is read again every round (kept in registers
// it would cost 64 of them), and the lane's place in it is worked out again:
// both are opaque to the optimiser, which would otherwise keep the addresses
// of the compare in registers over the K loop.
__device__ __forceinline__ void gp_compare_round(const f32x4 (&acc)[4][4],
                                                 const float* expected, int wm,
                                                 int wn, int lane, int round, GpVerdict& v) {
  int again = 0;
  asm volatile("" : "+s"(again), "+v"(lane));
  const int i16 = lane & 15, g = lane >> 4;
  // expected element of accumulator (i, j, r): want_lane[(16 i + r) * 128 + 16 j]
  const float* want_lane = expected + (wm * 64 + g * 4) * GP_TILE + wn * 64 + i16;
  const float* want = want_lane + again;
  unsigned bad = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const unsigned bits = __float_as_uint(acc[i][j][r]);
        bad += bits != __float_as_uint(want[(i * 16 + r) * GP_TILE + j * 16]);
        v.checksum ^= bits;
      }
    asm volatile("" ::: "memory");  // 16 expected values in registers at a time, not 64
  }
  bad = wave_add(bad);
  if (bad) {  // wave-uniform, and rare
    if (v.first_round < 0) {
      v.first_round = round;
      asm volatile("" : "+s"(again));  // a second read, not the first one's compare masks
      want = want_lane + again;
      unsigned index = 0xFFFFFFFFu;
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (__float_as_uint(acc[i][j][r]) !=
                __float_as_uint(want[(i * 16 + r) * GP_TILE + j * 16]))
              index = min(index, (unsigned)((i * 16 + g * 4 + r) * 64 + j * 16 + i16));
      v.first_index = wave_min(index);
    }
    v.mismatched += (int)bad;
  }
}

// the last round's tile to C[M,N]; m0, n0: the workgroup's first element. The
// lane is opaque for the reason gp_compare_round gives.
__device__ __forceinline__ void gp_store_c(const f32x4 (&acc)[4][4], float* C, int N,
                                           int m0, int n0, int wm, int wn, int lane) {
  asm volatile("" : "+v"(lane));
  const int i16 = lane & 15, g = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        C[(size_t)(m0 + wm * 64 + i * 16 + g * 4 + r) * N + n0 + wn * 64 + j * 16 + i16] =
            acc[i][j][r];
}

__device__ __forceinline__ void gp_store_record(int4* records, int wave, int lane,
                                                unsigned place, const GpVerdict& v) {
  const unsigned checksum = wave_xor(v.checksum);
  if (lane == 0)
    store_record8(records, blockIdx.x * 4 + wave, (int)place, v.mismatched, v.first_round,
                  (int)v.first_index, (int)checksum, 0, 0, 0);
}

template <int FMT, int BL>
__global__ void __launch_bounds__(256, 2)
gemm_pipe_kernel(const char* __restrict__ A, const char* __restrict__ B,
                 const float* __restrict__ expected, int4* __restrict__ records,
                 float* __restrict__ C, int N, int K, int tiles_n, int rounds, int store_c,
                 int inject_block, int inject_round) {
  __shared__ __attribute__((aligned(1024))) char gp_lds[GP_STAGES * GP_STAGE_BYTES];
  constexpr int ES = FMT == GP_BF16 ? 2 : 1;
  constexpr int BK = GP_STEP_BYTES / ES;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int i16 = lane & 15, g = lane >> 4;
  const int m0 = (blockIdx.x / tiles_n) * GP_TILE, n0 = (blockIdx.x % tiles_n) * GP_TILE;
  const unsigned place = hw_word();
  const int steps = K / BK;

  // where this lane's 16 bytes of each load come from, relative to the tile's
  // first byte of the step
  unsigned aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int t = wave * 4 + i;
    const int r = 8 * t + (lane >> 3), s = lane & 7;
    aoff[i] = (unsigned)r * (unsigned)(K * ES) + ((s ^ gp_key_b128(r)) << 4);
    if constexpr (BL == GP_NK) {
      boff[i] = aoff[i];
    } else if constexpr (FMT == GP_FP8) {
      boff[i] = (unsigned)r * (unsigned)N + ((s ^ gp_key_tr8(r)) << 4);
    } else {
      const int k = 4 * t + (lane >> 4), s16 = lane & 15;
      boff[i] = (unsigned)k * (unsigned)(2 * N) + ((s16 ^ (gp_key_tr16(k) << 1)) << 4);
    }
  }
  const char* a_tile = A + (size_t)m0 * K * ES;
  const char* b_tile = BL == GP_NK ? B + (size_t)n0 * K * ES : B + (size_t)n0 * ES;
  const size_t a_step = GP_STEP_BYTES;
  const size_t b_step = BL == GP_NK ? (size_t)GP_STEP_BYTES : (size_t)BK * N * ES;

  // LDS byte offsets of this lane's fragment reads inside a stage; bf16 kn:
  // tile t's first tr_b16 read
  unsigned a_at[2], b_at[4];
  gp_frag_addrs<BL>(a_at, b_at, wm, wn, i16, g);
  if constexpr (BL == GP_KN && FMT == GP_BF16) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int nb = wn * 64 + t * 16;
      const int k = g * 8 + (i16 >> 2);
      const int chunk = (nb >> 3) + ((i16 & 3) >> 1);
      b_at[t] = k * 256 + ((chunk ^ (gp_key_tr16(k) << 1)) << 4) + (i16 & 1) * 8;
    }
  }

  GP_LDS_AS char* lds = (GP_LDS_AS char*)gp_lds;
  const unsigned lds_base = (unsigned)reinterpret_cast<__UINTPTR_TYPE__>(lds);
  const bool inject_here = (int)blockIdx.x == inject_block && threadIdx.x == 0;
  GpVerdict verdict;
  f32x4 acc[4][4];
  for (int round = 0; round < rounds; round++) {
    GP_ZERO_ACC(acc)
    const char* a_src = a_tile;
    const char* b_src = b_tile;
    // stage 0 may still be read by a wave that is finishing the last round
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    gp_issue(a_src, b_src, aoff, boff, lds, wave);
    for (int k = 0; k < steps; k++) {
      // barrier 1: the other stage has been read for the last time
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (k + 1 < steps) {
        a_src += a_step;
        b_src += b_step;
        gp_issue(a_src, b_src, aoff, boff, lds + ((k + 1) & 1) * GP_STAGE_BYTES, wave);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // step k+1's eight stay in flight
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // barrier 2: every wave's part of step k has landed
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const unsigned sa = lds_base + (k & 1) * GP_STAGE_BYTES;
      GpFrags<BL> f0, f1;
      unsigned b0[4], b1[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        b0[t] = sa + b_at[BL == GP_NK ? 0 : t];
        b1[t] = sa + b_at[BL == GP_NK ? 1 : t];
      }
      gp_read_half<FMT, BL, 0>(f0, sa + a_at[0], b0);
      gp_read_half<FMT, BL, 1>(f1, sa + a_at[1], b1);
      gp_wait_half<BL, true>(f0);  // the second half's reads stay in flight
      gp_mma_half<FMT, BL>(f0, acc);
      __builtin_amdgcn_sched_barrier(0);  // the first half's MFMAs stay above the wait
      gp_wait_half<BL, false>(f1);
      gp_mma_half<FMT, BL>(f1, acc);
    }
    if (inject_here && round == inject_round) gp_inject(acc);
    gp_compare_round(acc, expected, wm, wn, lane, round, verdict);
  }
  if (store_c) gp_store_c(acc, C, N, m0, n0, wm, wn, lane);
  gp_store_record(records, wave, lane, place, verdict);
}

// image: int32, at most 16 KiB, on the current GPU; addrs: 64 int32 byte
// addresses into it, one per lane (any device: they are checked on the host).
// Returns int32 [64,2] ([64,3] for width 6).
torch::Tensor lds_tr_read(long width, torch::Tensor image, torch::Tensor addrs) {
  TORCH_CHECK(width == 16 || width == 8 || width == 4 || width == 6,
              "width must be one of 16, 8, 4, 6; got ", width);
  TORCH_CHECK(image.is_cuda() && image.dtype() == torch::kInt32 && image.dim() == 1 &&
                  image.is_contiguous() && image.numel() >= 1 &&
                  image.numel() <= TR_IMAGE_MAX_WORDS,
              "image must be a contiguous 1-D int32 GPU tensor of 1..4096 words");
  TORCH_CHECK(addrs.dtype() == torch::kInt32 && addrs.numel() == 64,
              "addrs must hold 64 int32 byte addresses (one per lane)");
  const long bytes = 4 * image.numel();
  const long span = width == 6 ? 12 : 8, align = width == 6 ? 16 : 8;
  auto host = addrs.cpu().contiguous();
  const int* a = host.data_ptr<int>();
  for (int l = 0; l < 64; l++) {
    TORCH_CHECK(a[l] >= 0 && a[l] + span <= bytes, "addrs[", l, "] = ", a[l],
                " reads outside the image of ", bytes, " bytes");
    TORCH_CHECK(a[l] % align == 0, "addrs[", l, "] = ", a[l], " is not ", align,
                "-byte aligned");
  }
  auto dev_addrs = host.to(image.device());
  auto regs = torch::zeros({64, width == 6 ? 3 : 2}, image.options());
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto width_c) {
    hipLaunchKernelGGL((lds_tr_read_kernel<decltype(width_c)::value>), dim3(1), dim3(64), 0,
                       stream, image.data_ptr<int>(), (int)image.numel(),
                       dev_addrs.data_ptr<int>(), regs.data_ptr<int>());
  };
  if (width == 16) launch(std::integral_constant<int, 16>{});
  else if (width == 8) launch(std::integral_constant<int, 8>{});
  else if (width == 4) launch(std::integral_constant<int, 4>{});
  else launch(std::integral_constant<int, 6>{});
  HIP_CHECK(hipGetLastError());
  return regs;
}

// What the wrappers of the three tiled GEMM probes share once M, N and K are
// known: the kernels' common argument tail with the records and C it points to.
struct GpRun {
  torch::Tensor expected, records, C;
  long N, K, tiles_n, grid, rounds, inject_block, inject_round;
  bool store_c;
};

// Checks expected, the tiling, the length of the run and the injection,
// leaves A and B contiguous and 16-byte aligned, allocates records and C.
static GpRun gp_prepare(torch::Tensor& A, torch::Tensor& B, const torch::Tensor& expected, long M,
                        long N, long K, long rounds, bool store_c, long inject_block,
                        long inject_round) {
  TORCH_CHECK(expected.dtype() == torch::kFloat32 &&
                  expected.sizes() == torch::IntArrayRef({GP_TILE, GP_TILE}),
              "expected must be float32 [128,128]");
  TORCH_CHECK(M >= GP_TILE && N >= GP_TILE && M % GP_TILE == 0 && N % GP_TILE == 0,
              "M and N must be positive multiples of 128; got ", M, ", ", N);
  const long tiles_n = N / GP_TILE, grid = (M / GP_TILE) * tiles_n;
  TORCH_CHECK(rounds >= 1, "rounds must be >= 1");
  // bounded run: 2^33 tile-K-elements are 2.8e14 FLOP, about a second at the
  // rate the pipeline reaches (BENCHMARKS.md "GEMM probe")
  TORCH_CHECK(grid <= (1L << 20) && rounds <= (1L << 22) && rounds * K * grid <= (1L << 33),
              "rounds*K*grid must be <= 2^33; got ", rounds, "*", K, "*", grid);
  TORCH_CHECK(inject_block >= -1 && inject_block < grid && inject_round >= -1 &&
                  inject_round < rounds,
              "inject_block/inject_round out of range");
  A = A.contiguous();
  B = B.contiguous();
  // a direct-to-LDS load fetches 16 aligned bytes (mx6 B kn: 4); every row
  // pitch is a multiple of 16
  TORCH_CHECK(reinterpret_cast<uintptr_t>(A.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(B.data_ptr()) % 16 == 0,
              "A and B must be 16-byte aligned");
  GpRun run;
  run.expected = expected.contiguous();
  run.records = zero_records(grid * 4, 8, A.device());
  run.C = store_c ? torch::zeros({M, N}, expected.options())
                  : torch::empty({0}, expected.options());
  run.N = N, run.K = K, run.tiles_n = tiles_n, run.grid = grid, run.rounds = rounds;
  run.inject_block = inject_block, run.inject_round = inject_round, run.store_c = store_c;
  return run;
}

// `lead`: the kernel's arguments in front of the common tail (A, B, the scales)
template <typename Kernel, typename... Lead>
static void gp_launch(Kernel kernel, const GpRun& run, hipStream_t stream, Lead... lead) {
  hipLaunchKernelGGL(kernel, dim3(run.grid), dim3(256), 0, stream, lead...,
                     run.expected.data_ptr<float>(),
                     reinterpret_cast<int4*>(run.records.data_ptr<int>()),
                     run.store_c ? run.C.data_ptr<float>() : nullptr, (int)run.N, (int)run.K,
                     (int)run.tiles_n, (int)run.rounds, (int)run.store_c, (int)run.inject_block,
                     (int)run.inject_round);
}

// A [M,K]; B [K,N] (b_layout "kn") or [N,K] ("nk"); fmt "bf16": bfloat16
// tensors, "fp8": uint8 raw e4m3 bytes; expected [128,128] fp32, the tile every
// workgroup must compute. One untimed warm-up launch, then one timed launch
// (warm_then_timed_ms). Returns (records [grid*4,8] int32, C [M,N] fp32 when
// store_c else an empty tensor, elapsed_ms of the timed launch).
std::tuple<torch::Tensor, torch::Tensor, double> gemm_pipe(
    torch::Tensor A, torch::Tensor B, torch::Tensor expected, const std::string& fmt,
    const std::string& b_layout, long rounds, bool store_c, long inject_block,
    long inject_round) {
  const int f = fmt == "bf16" ? GP_BF16 : fmt == "fp8" ? GP_FP8 : -1;
  TORCH_CHECK(f >= 0, "fmt must be one of bf16, fp8; got ", fmt);
  const int bl = b_layout == "kn" ? GP_KN : b_layout == "nk" ? GP_NK : -1;
  TORCH_CHECK(bl >= 0, "b_layout must be one of kn, nk; got ", b_layout);
  TORCH_CHECK(A.is_cuda() && B.is_cuda() && expected.is_cuda(), "A/B/expected must be on GPU");
  TORCH_CHECK(A.device() == B.device() && A.device() == expected.device(),
              "A/B/expected must be on the same device");
  if (f == GP_BF16) {
    TORCH_CHECK(A.dtype() == torch::kBFloat16 && B.dtype() == torch::kBFloat16,
                "bf16: A/B must be bfloat16");
  } else {
    TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8,
                "fp8: A/B must be uint8 (raw e4m3 bytes)");
  }
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2, "A and B must be 2-D");
  const long M = A.size(0), K = A.size(1);
  const long N = bl == GP_KN ? B.size(1) : B.size(0);
  TORCH_CHECK((bl == GP_KN ? B.size(0) : B.size(1)) == K, "B must be ",
              bl == GP_KN ? "[K,N]" : "[N,K]", " with K=", K);
  const long BK = f == GP_BF16 ? 64 : 128;
  TORCH_CHECK(K >= BK && K % BK == 0, "K must be a positive multiple of ", BK, "; got ", K);
  // |operand| <= 2, so every partial sum is an integer <= 4*K: exact in fp32
  // only up to 2^24. For fp8 it is also inside the window the pipe keeps
  // within a lane group (BENCHMARKS.md "the fp8 pipes are narrower than fp32":
  // a product up to 13 bits below the group's largest survives; here all
  // products are integers of at most 3 bits)
  TORCH_CHECK(4 * K <= (1L << 24), "K ", K, " breaks fp32 exactness (need 4*K <= 2^24)");
  // the kernel's per-lane offsets into a tile's rows are 32-bit
  TORCH_CHECK(M <= (1L << 22) && N <= (1L << 22), "M and N must be <= 2^22");
  const GpRun run =
      gp_prepare(A, B, expected, M, N, K, rounds, store_c, inject_block, inject_round);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<4>(2 * f + bl, [&](auto case_c) {
      constexpr int c = decltype(case_c)::value;
      gp_launch(gemm_pipe_kernel<c / 2, c % 2>, run, stream,
                static_cast<const char*>(A.data_ptr()), static_cast<const char*>(B.data_ptr()));
    });
  });
  return std::make_tuple(run.records, run.C, ms);
}

// ---------------------------------------------------------------------------
// MX GEMM probe: gemm_pipe's pipeline feeding v_mfma_scale_f32_16x16x128_f8f6f4,
// the GEMM an MXFP8 / MXFP4 tenant runs: C = (A o scales).(B o scales), fp32
// accumulate, every 32 elements of K of a row of A or a column of B under one
// E8M0 byte that is streamed from memory next to the operands. The MX scale
// probe above runs this instruction from registers only; here the scaled pipe,
// the direct-to-LDS loads, the LDS fragment reads (4-bit and 8-bit transpose
// reads for B kn) and the scale loads are busy in the same cycles, and every
// tile is compared bitwise in registers (operands: ops/mx_gemm_probe.py).
//
// FMT mxfp8: e4m3 both sides, one code per byte. mxfp4: e2m1 both sides, two
// codes per byte, the even element in the low nibble; the packed dimension is
// K for A [M,K] and B nk [N,K], N for B kn [K,N]. scale_a [M,K/32]; scale_b
// [N,K/32] (nk) or [K/32,N] (kn): plain row-major bytes, not pre-shuffled.
//
// Same shape as gemm_pipe_kernel, to be read side by side with it: one
// workgroup of 256 threads per 128x128 tile of C, waves 2x2, 4x4 MFMA tiles
// per wave, 64 accumulator registers held for the whole K loop, two LDS stages
// of 32 KiB (A tile at 0, B tile at 16 KiB), eight global_load_lds_dwordx4 per
// wave and K step with the swizzle on the source side, barrier 1 / issue step
// k+1 / wait / barrier 2 / read / MFMA. A K step is 128 bytes per row: 128
// e4m3 elements, one scaled MFMA deep, or 256 e2m1 elements, two deep (K
// chunk 0 is bytes 0..63 of the row, chunk 1 bytes 64..127).
//
// Fragments. Lane (i, g) of a 16x16x128 tile holds, 4-bit: the 16 bytes with
// k = 32g..32g+31 of its K chunk (VGPRs 0-3; the operand's upper four are not
// read); 8-bit: k = 16g..16g+15 in VGPRs 0-3 and k = 64+16g.. in VGPRs 4-7
// (the measured walk, see "MX scale probe"). For A and B nk that is, in both
// formats, the 16-byte chunks g and g+4 of the row: gemm_pipe's ds_read_b128
// addressing and key, chunk g+4 at address ^ 64. fp4 uses them as two MFMAs,
// fp8 as the two halves of one operand.
//   B kn fp8: the tile is 128 k rows of 128 bytes; ds_read_b64_tr_b8 gives 8 k
//     per read, two reads 16 consecutive k, the second half 64 rows on:
//     gemm_pipe's fp8 kn map and key, the four reads forming one operand.
//   B kn fp4: the tile is 256 k rows of 64 bytes (128 nibbles of n). A load of
//     1 KiB lands 16 rows of four 16-byte slots. ds_read_b64_tr_b4: a group of
//     16 lanes addresses 16 k rows, lane i the 8 bytes (16 nibbles, one 16x16
//     tile's columns) of row 128c + 32g + 16h + i for read h of chunk c, and
//     receives column i, 16 consecutive k, lowest first; two reads are the
//     lane's 32 k. Tile t of wave column wn is 8-byte unit 4 wn + t of the
//     row: slot (2 wn + (t>>1)) ^ key, half t & 1.
//   fp4 kn key = (k>>2) & 3. Rows of 64 bytes: four rows fill the 64 banks, so
//     rows k and k+4 collide. Every lane of one read takes the same half of its
//     16-byte slot (the load lands 16 bytes whole, so the source-side swizzle
//     cannot move a half), hence 32 lanes reach at most 32 banks: the degree
//     is 2 at best. Assuming one LDS pass serves 32 consecutive lanes of a b64
//     read (rows 32g..32g+15 and 32g+32..32g+47): the eight rows that share
//     k & 3 fall on the four slots by (k>>2) & 3, two each. Conflict degree 2
//     by construction under that assumption; not measured with counters.
//
// Scales. Block b of a tile's K chunk is scaled by the byte lane group b
// supplies, in every format, so lane (i, g) supplies per K chunk the byte of
// (row 16 t + i, block g) for each of its four A tiles t and four B tiles.
// They are fetched with global_load_ubyte (inline assembly, so that their
// number and place in the vmcnt order are the source's, not the compiler's):
// four A and four B loads per chunk, 8 (fp8) or 16 (fp4) per step, a step
// ahead of use, gathered after the wait into the four bytes of one VGPR per
// side and chunk (shifts and ors); the MFMA of tile (t_a, t_b) selects its
// bytes with op_sel = t_a and t_b, immediates in the unrolled tile loop. No
// LDS is spent on scales. Nothing is indexed by a loaded value.
//
// vmcnt, from the loads in flight, oldest first. Before the loop: LDS(0) [8],
// scales(0) [S]. Step k: after barrier 1, LDS(k+1) [8] is issued; in flight
// are LDS(k), scales(k), LDS(k+1), and s_waitcnt vmcnt(8) leaves exactly
// LDS(k+1) in flight: step k's operands have landed and its scale bytes are
// in registers. They are gathered, and only then scales(k+1) [S] is issued
// into the same registers, behind LDS(k+1), which restores the order for step
// k+1. The last step issues nothing and waits vmcnt(0). There is no other
// vmcnt wait in the K loop, and every step loads its own scale bytes.
//
// lgkmcnt. fp4: as gemm_pipe, the two K chunks are two halves: all reads are
// issued, lgkmcnt(8) (kn: 12) before chunk 0's 16 MFMAs, lgkmcnt(0) before
// chunk 1's. fp8: one MFMA consumes both pieces, so the step is split by
// tiles: B's reads (nk 8, kn 16) and A tiles 0-1 (4) are issued, then A tiles
// 2-3 (4); lgkmcnt(4) before the 8 MFMAs of A tiles 0-1, lgkmcnt(0) before the
// 8 of A tiles 2-3.
//
// Verification, records, store_c and inject are gemm_pipe's, by the same
// helpers (see "Verification in registers" there). Race and bounds:
// no wave waits for another workgroup; every loop bound is a launch argument;
// the wrapper fixes every shape the offsets are computed from. Build for
// gfx950 (register counts in BENCHMARKS.md "MX GEMM probe"): no scratch,
// 64 KiB of LDS, two workgroups per CU.
// ---------------------------------------------------------------------------
enum { MXG_FP8 = 0, MXG_FP4 = 1 };

__device__ __forceinline__ int mxg_key_tr4(int k) { return (k >> 2) & 3; }

#define MXG_READ(INSN, DST, AT, OFF) \
  asm volatile(INSN " %0, %1 offset:" #OFF : "=v"(DST) : "v"(AT) : "memory")
// one scale byte: base (wave-uniform) + off (per lane) + OFF; tied, so the
// next step's byte returns into the register the last one was gathered from
#define MXG_LOAD_SCALE(DST, VOFF, BASE, OFF)                           \
  asm volatile("global_load_ubyte %0, %1, %2 offset:" #OFF             \
               : "+v"(DST)                                             \
               : "v"(VOFF), "s"(BASE)                                  \
               : "memory")

// the lane's scale loads of one step. sa, sb: the step's first scale byte of
// the workgroup's rows (columns); a_off, b_off: this lane's (row i, block g) of
// tile 0 from there. A, B nk: tile t is 16 rows = `stride` bytes on (added to
// the wave-uniform base), K chunk 1 four blocks = 4 bytes on. B kn: the tiles
// are 16 columns apart in one row of scale_b, chunk 1 four rows = `stride` on.
template <int FMT, int BL>
__device__ __forceinline__ void mxg_load_scales(unsigned (&ra)[2][4], unsigned (&rb)[2][4],
                                                const unsigned char* sa, const unsigned char* sb,
                                                unsigned a_off, unsigned b_off, size_t a_stride,
                                                size_t b_stride) {
  const unsigned char* sa1 = sa + a_stride;
  const unsigned char* sa2 = sa1 + a_stride;
  const unsigned char* sa3 = sa2 + a_stride;
  const unsigned char* sb1 = sb + b_stride;
  MXG_LOAD_SCALE(ra[0][0], a_off, sa, 0);
  MXG_LOAD_SCALE(ra[0][1], a_off, sa1, 0);
  MXG_LOAD_SCALE(ra[0][2], a_off, sa2, 0);
  MXG_LOAD_SCALE(ra[0][3], a_off, sa3, 0);
  if constexpr (FMT == MXG_FP4) {
    MXG_LOAD_SCALE(ra[1][0], a_off, sa, 4);
    MXG_LOAD_SCALE(ra[1][1], a_off, sa1, 4);
    MXG_LOAD_SCALE(ra[1][2], a_off, sa2, 4);
    MXG_LOAD_SCALE(ra[1][3], a_off, sa3, 4);
  }
  if constexpr (BL == GP_NK) {
    const unsigned char* sb2 = sb1 + b_stride;
    const unsigned char* sb3 = sb2 + b_stride;
    MXG_LOAD_SCALE(rb[0][0], b_off, sb, 0);
    MXG_LOAD_SCALE(rb[0][1], b_off, sb1, 0);
    MXG_LOAD_SCALE(rb[0][2], b_off, sb2, 0);
    MXG_LOAD_SCALE(rb[0][3], b_off, sb3, 0);
    if constexpr (FMT == MXG_FP4) {
      MXG_LOAD_SCALE(rb[1][0], b_off, sb, 4);
      MXG_LOAD_SCALE(rb[1][1], b_off, sb1, 4);
      MXG_LOAD_SCALE(rb[1][2], b_off, sb2, 4);
      MXG_LOAD_SCALE(rb[1][3], b_off, sb3, 4);
    }
  } else {
    MXG_LOAD_SCALE(rb[0][0], b_off, sb, 0);
    MXG_LOAD_SCALE(rb[0][1], b_off, sb, 16);
    MXG_LOAD_SCALE(rb[0][2], b_off, sb, 32);
    MXG_LOAD_SCALE(rb[0][3], b_off, sb, 48);
    if constexpr (FMT == MXG_FP4) {
      MXG_LOAD_SCALE(rb[1][0], b_off, sb1, 0);
      MXG_LOAD_SCALE(rb[1][1], b_off, sb1, 16);
      MXG_LOAD_SCALE(rb[1][2], b_off, sb1, 32);
      MXG_LOAD_SCALE(rb[1][3], b_off, sb1, 48);
    }
  }
}
#undef MXG_LOAD_SCALE

// the step's vmcnt wait; names the scale registers it makes valid. MORE: step
// k+1's eight direct loads were issued after them and stay in flight
template <int FMT, bool MORE>
__device__ __forceinline__ void mxg_wait_vm(unsigned (&ra)[2][4], unsigned (&rb)[2][4]) {
#define MXG_WAIT_VM(CNT)                                                                    \
  if constexpr (FMT == MXG_FP8)                                                             \
    asm volatile("s_waitcnt vmcnt(" CNT ")"                                                 \
                 : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[0][2]), "+v"(ra[0][3]),          \
                   "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3])::"memory"); \
  else                                                                                      \
    asm volatile("s_waitcnt vmcnt(" CNT ")"                                                 \
                 : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[0][2]), "+v"(ra[0][3]),          \
                   "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3]),          \
                   "+v"(ra[1][0]), "+v"(ra[1][1]), "+v"(ra[1][2]), "+v"(ra[1][3]),          \
                   "+v"(rb[1][0]), "+v"(rb[1][1]), "+v"(rb[1][2]), "+v"(rb[1][3])::"memory")
  if constexpr (MORE) { MXG_WAIT_VM("8"); }
  else { MXG_WAIT_VM("0"); }
#undef MXG_WAIT_VM
}
__device__ __forceinline__ int mxg_gather(const unsigned (&r)[4]) {
  return (int)(r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24));
}

// the 16 MFMAs of A tiles I0.. x all B tiles; op_sel must be an immediate
#define MXG_MMA(FMT_CODE, I, J)                                                          \
  acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[I], b[J], acc[I][J],    \
                                                               FMT_CODE, FMT_CODE, I, sa, J, sb)
#define MXG_MMA_ROW(FMT_CODE, I) \
  MXG_MMA(FMT_CODE, I, 0); MXG_MMA(FMT_CODE, I, 1); MXG_MMA(FMT_CODE, I, 2); MXG_MMA(FMT_CODE, I, 3)

// fp4: one K chunk = one half of the step, as gp_read_half / gp_wait_half
template <int BL> struct MxgFrags4 {
  gp_i4 a[4];
  gp_i4 b[4];            // nk
  gp_i2 lo[4], hi[4];    // kn: k 0..15 and 16..31 of the lane's 32
};
template <int BL, int HS>
__device__ __forceinline__ void mxg_read_half4(MxgFrags4<BL>& f, unsigned a_at,
                                               const unsigned (&b_at)[4]) {
  MXG_READ("ds_read_b128", f.a[0], a_at, 0);
  MXG_READ("ds_read_b128", f.a[1], a_at, 2048);
  MXG_READ("ds_read_b128", f.a[2], a_at, 4096);
  MXG_READ("ds_read_b128", f.a[3], a_at, 6144);
  if constexpr (BL == GP_NK) {
    MXG_READ("ds_read_b128", f.b[0], b_at[0], 16384);
    MXG_READ("ds_read_b128", f.b[1], b_at[0], 18432);
    MXG_READ("ds_read_b128", f.b[2], b_at[0], 20480);
    MXG_READ("ds_read_b128", f.b[3], b_at[0], 22528);
  } else {
    // chunk 1 is 128 k rows = 8192 bytes on; hi is 16 rows = 1024 on
#pragma unroll
    for (int t = 0; t < 4; t++) {
      if constexpr (HS == 0) {
        MXG_READ("ds_read_b64_tr_b4", f.lo[t], b_at[t], 16384);
        MXG_READ("ds_read_b64_tr_b4", f.hi[t], b_at[t], 17408);
      } else {
        MXG_READ("ds_read_b64_tr_b4", f.lo[t], b_at[t], 24576);
        MXG_READ("ds_read_b64_tr_b4", f.hi[t], b_at[t], 25600);
      }
    }
  }
}
template <int BL, bool OTHERS>
__device__ __forceinline__ void mxg_wait_half4(MxgFrags4<BL>& f) {
  if constexpr (BL == GP_NK) {
#define MXG_WAIT_NK(CNT)                                                                    \
  asm volatile("s_waitcnt lgkmcnt(" CNT ")"                                                 \
               : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]),      \
                 "+v"(f.b[1]), "+v"(f.b[2]), "+v"(f.b[3])::"memory")
    if constexpr (OTHERS) MXG_WAIT_NK("8");
    else MXG_WAIT_NK("0");
#undef MXG_WAIT_NK
  } else {
#define MXG_WAIT_KN(CNT)                                                                    \
  asm volatile("s_waitcnt lgkmcnt(" CNT ")"                                                 \
               : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.lo[0]),     \
                 "+v"(f.lo[1]), "+v"(f.lo[2]), "+v"(f.lo[3]), "+v"(f.hi[0]), "+v"(f.hi[1]), \
                 "+v"(f.hi[2]), "+v"(f.hi[3])::"memory")
    if constexpr (OTHERS) MXG_WAIT_KN("12");
    else MXG_WAIT_KN("0");
#undef MXG_WAIT_KN
  }
}
template <int BL>
__device__ __forceinline__ void mxg_mma_half4(const MxgFrags4<BL>& f, f32x4 (&acc)[4][4], int sa,
                                              int sb) {
  const gp_i4 zero = {0, 0, 0, 0};  // the 4-bit form reads VGPRs 0-3 only
  i32x8 a[4], b[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    a[t] = __builtin_shufflevector(f.a[t], zero, 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (BL == GP_NK)
      b[t] = __builtin_shufflevector(f.b[t], zero, 0, 1, 2, 3, 4, 5, 6, 7);
    else
      b[t] = __builtin_shufflevector(__builtin_shufflevector(f.lo[t], f.hi[t], 0, 1, 2, 3), zero,
                                     0, 1, 2, 3, 4, 5, 6, 7);
  }
  MXG_MMA_ROW(4, 0);
  MXG_MMA_ROW(4, 1);
  MXG_MMA_ROW(4, 2);
  MXG_MMA_ROW(4, 3);
}

// fp8: the whole step's fragments, split by A tiles
template <int BL> struct MxgFrags8 {
  gp_i4 a[4][2];         // chunks g and g+4
  gp_i4 b[4][2];         // nk
  gp_i2 tr[4][4];        // kn: k 16g.., 16g+8.., 64+16g.., 64+16g+8..
};
template <int BL>
// a_at: the lane's chunks g and g+4 of A tile 0; nk: b_at[0], b_hi[0] likewise
// of B tile 0; kn: b_at[t] tile t's first read
__device__ __forceinline__ void mxg_read_step8(MxgFrags8<BL>& f, const unsigned (&a_at)[2],
                                               const unsigned (&b_at)[4],
                                               const unsigned (&b_hi)[4]) {
  if constexpr (BL == GP_NK) {
    MXG_READ("ds_read_b128", f.b[0][0], b_at[0], 16384);
    MXG_READ("ds_read_b128", f.b[0][1], b_hi[0], 16384);
    MXG_READ("ds_read_b128", f.b[1][0], b_at[0], 18432);
    MXG_READ("ds_read_b128", f.b[1][1], b_hi[0], 18432);
    MXG_READ("ds_read_b128", f.b[2][0], b_at[0], 20480);
    MXG_READ("ds_read_b128", f.b[2][1], b_hi[0], 20480);
    MXG_READ("ds_read_b128", f.b[3][0], b_at[0], 22528);
    MXG_READ("ds_read_b128", f.b[3][1], b_hi[0], 22528);
  } else {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      MXG_READ("ds_read_b64_tr_b8", f.tr[t][0], b_at[t], 16384);
      MXG_READ("ds_read_b64_tr_b8", f.tr[t][1], b_at[t], 17408);
      MXG_READ("ds_read_b64_tr_b8", f.tr[t][2], b_at[t], 24576);
      MXG_READ("ds_read_b64_tr_b8", f.tr[t][3], b_at[t], 25600);
    }
  }
  MXG_READ("ds_read_b128", f.a[0][0], a_at[0], 0);
  MXG_READ("ds_read_b128", f.a[0][1], a_at[1], 0);
  MXG_READ("ds_read_b128", f.a[1][0], a_at[0], 2048);
  MXG_READ("ds_read_b128", f.a[1][1], a_at[1], 2048);
  MXG_READ("ds_read_b128", f.a[2][0], a_at[0], 4096);
  MXG_READ("ds_read_b128", f.a[2][1], a_at[1], 4096);
  MXG_READ("ds_read_b128", f.a[3][0], a_at[0], 6144);
  MXG_READ("ds_read_b128", f.a[3][1], a_at[1], 6144);
}
// part 0: B and A tiles 0-1 have returned, the four reads of A tiles 2-3 may
// stay in flight; part 1: everything has
template <int BL, int PART>
__device__ __forceinline__ void mxg_wait_part8(MxgFrags8<BL>& f) {
  if constexpr (PART == 1) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(f.a[2][0]), "+v"(f.a[2][1]), "+v"(f.a[3][0]), "+v"(f.a[3][1])::"memory");
  } else if constexpr (BL == GP_NK) {
    asm volatile("s_waitcnt lgkmcnt(4)"
                 : "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]),
                   "+v"(f.b[0][0]), "+v"(f.b[0][1]), "+v"(f.b[1][0]), "+v"(f.b[1][1]),
                   "+v"(f.b[2][0]), "+v"(f.b[2][1]), "+v"(f.b[3][0]), "+v"(f.b[3][1])::"memory");
  } else {
    asm volatile("s_waitcnt lgkmcnt(4)"
                 : "+v"(f.a[0][0]), "+v"(f.a[0][1]), "+v"(f.a[1][0]), "+v"(f.a[1][1]),
                   "+v"(f.tr[0][0]), "+v"(f.tr[0][1]), "+v"(f.tr[0][2]), "+v"(f.tr[0][3]),
                   "+v"(f.tr[1][0]), "+v"(f.tr[1][1]), "+v"(f.tr[1][2]), "+v"(f.tr[1][3]),
                   "+v"(f.tr[2][0]), "+v"(f.tr[2][1]), "+v"(f.tr[2][2]), "+v"(f.tr[2][3]),
                   "+v"(f.tr[3][0]), "+v"(f.tr[3][1]), "+v"(f.tr[3][2]), "+v"(f.tr[3][3])::"memory");
  }
}
template <int BL, int PART>
__device__ __forceinline__ void mxg_mma_part8(const MxgFrags8<BL>& f, f32x4 (&acc)[4][4], int sa,
                                              int sb) {
  i32x8 a[4], b[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    a[t] = __builtin_shufflevector(f.a[t][0], f.a[t][1], 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (BL == GP_NK)
      b[t] = __builtin_shufflevector(f.b[t][0], f.b[t][1], 0, 1, 2, 3, 4, 5, 6, 7);
    else
      b[t] = __builtin_shufflevector(__builtin_shufflevector(f.tr[t][0], f.tr[t][1], 0, 1, 2, 3),
                                     __builtin_shufflevector(f.tr[t][2], f.tr[t][3], 0, 1, 2, 3),
                                     0, 1, 2, 3, 4, 5, 6, 7);
  }
  if constexpr (PART == 0) {
    MXG_MMA_ROW(0, 0);
    MXG_MMA_ROW(0, 1);
  } else {
    MXG_MMA_ROW(0, 2);
    MXG_MMA_ROW(0, 3);
  }
}
#undef MXG_READ
#undef MXG_MMA_ROW
#undef MXG_MMA

template <int FMT, int BL>
__global__ void __launch_bounds__(256, 2)
mx_gemm_pipe_kernel(const char* __restrict__ A, const char* __restrict__ B,
                    const unsigned char* __restrict__ scale_a,
                    const unsigned char* __restrict__ scale_b, const float* __restrict__ expected,
                    int4* __restrict__ records, float* __restrict__ C, int N, int K, int tiles_n,
                    int rounds, int store_c, int inject_block, int inject_round) {
  __shared__ __attribute__((aligned(1024))) char mxg_lds[GP_STAGES * GP_STAGE_BYTES];
  constexpr int BK = FMT == MXG_FP8 ? GP_STEP_BYTES : 2 * GP_STEP_BYTES;  // elements per step
  constexpr int STEP_BLOCKS = BK / 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int i16 = lane & 15, g = lane >> 4;
  const int m0 = (blockIdx.x / tiles_n) * GP_TILE, n0 = (blockIdx.x % tiles_n) * GP_TILE;
  const unsigned place = hw_word();
  const int steps = K / BK;
  const unsigned row_bytes = FMT == MXG_FP8 ? (unsigned)K : (unsigned)K >> 1;  // A, B nk
  const unsigned n_bytes = FMT == MXG_FP8 ? (unsigned)N : (unsigned)N >> 1;    // B kn
  const unsigned kblocks = (unsigned)K >> 5;

  // where this lane's 16 bytes of each load come from, relative to the tile's
  // first byte of the step
  unsigned aoff[4], boff[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int t = wave * 4 + i;
    const int r = 8 * t + (lane >> 3), s = lane & 7;
    aoff[i] = (unsigned)r * row_bytes + ((s ^ gp_key_b128(r)) << 4);
    if constexpr (BL == GP_NK) {
      boff[i] = aoff[i];
    } else if constexpr (FMT == MXG_FP8) {
      boff[i] = (unsigned)r * n_bytes + ((s ^ gp_key_tr8(r)) << 4);
    } else {
      const int k = 16 * t + (lane >> 2), s4 = lane & 3;
      boff[i] = (unsigned)k * n_bytes + ((s4 ^ mxg_key_tr4(k)) << 4);
    }
  }
  const char* a_tile = A + (size_t)m0 * row_bytes;
  const char* b_tile = BL == GP_NK ? B + (size_t)n0 * row_bytes
                                   : B + (FMT == MXG_FP8 ? n0 : n0 >> 1);
  const size_t a_step = GP_STEP_BYTES;
  const size_t b_step = BL == GP_NK ? (size_t)GP_STEP_BYTES : (size_t)BK * n_bytes;

  // the lane's scale bytes of a step, relative to the step's first byte of the
  // workgroup's rows (columns); a step is STEP_BLOCKS bytes (kn: rows) on
  // (tile 0; the other tiles and K chunk 1 are wave-uniform strides on)
  const unsigned sa_off = (unsigned)(wm * 64 + i16) * kblocks + g;
  const unsigned sb_off = BL == GP_NK ? (unsigned)(wn * 64 + i16) * kblocks + g
                                      : (unsigned)g * (unsigned)N + wn * 64 + i16;
  const size_t sa_stride = (size_t)16 * kblocks;
  const size_t sb_stride = BL == GP_NK ? (size_t)16 * kblocks : (size_t)4 * N;
  const unsigned char* sa_tile = scale_a + (size_t)m0 * kblocks;
  const unsigned char* sb_tile = BL == GP_NK ? scale_b + (size_t)n0 * kblocks : scale_b + n0;
  const size_t sa_step = STEP_BLOCKS;
  const size_t sb_step = BL == GP_NK ? (size_t)STEP_BLOCKS : (size_t)STEP_BLOCKS * N;

  // LDS byte offsets of this lane's fragment reads inside a stage, as in
  // gemm_pipe_kernel; fp4 kn: per tile, the chunk and the read are immediates
  unsigned a_at[2], b_at[4];
  gp_frag_addrs<BL>(a_at, b_at, wm, wn, i16, g);
  if constexpr (BL == GP_KN && FMT == MXG_FP4) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int k = g * 32 + i16;
      b_at[t] = k * 64 + (((wn * 2 + (t >> 1)) ^ mxg_key_tr4(k)) << 4) + (t & 1) * 8;
    }
  }

  GP_LDS_AS char* lds = (GP_LDS_AS char*)mxg_lds;
  const unsigned lds_base = (unsigned)reinterpret_cast<__UINTPTR_TYPE__>(lds);
  const bool inject_here = (int)blockIdx.x == inject_block && threadIdx.x == 0;
  GpVerdict verdict;
  unsigned raw_a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, raw_b[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  f32x4 acc[4][4];
  for (int round = 0; round < rounds; round++) {
    GP_ZERO_ACC(acc)
    const char* a_src = a_tile;
    const char* b_src = b_tile;
    const unsigned char* sa_src = sa_tile;
    const unsigned char* sb_src = sb_tile;
    // stage 0 may still be read by a wave that is finishing the last round
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    gp_issue(a_src, b_src, aoff, boff, lds, wave);
    mxg_load_scales<FMT, BL>(raw_a, raw_b, sa_src, sb_src, sa_off, sb_off, sa_stride,
                             sb_stride);
    // one K step. MORE: not the last one. The last step is peeled off the loop
    // so that the loop body has no branch: the scale registers then form one
    // chain of tied operands (load, wait, load, ...) that the compiler keeps in
    // place; a copy of a register with a load in flight would read stale bytes
    auto step = [&](auto more_c, int k) {
      constexpr bool MORE = decltype(more_c)::value;
      // barrier 1: the other stage has been read for the last time
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if constexpr (MORE) {
        a_src += a_step;
        b_src += b_step;
        gp_issue(a_src, b_src, aoff, boff, lds + ((k + 1) & 1) * GP_STAGE_BYTES, wave);
      }
      // step k's operands and scales are in; step k+1's eight stay in flight
      mxg_wait_vm<FMT, MORE>(raw_a, raw_b);
      const int sa0 = mxg_gather(raw_a[0]), sb0 = mxg_gather(raw_b[0]);
      [[maybe_unused]] int sa1 = 0, sb1 = 0;
      if constexpr (FMT == MXG_FP4) {
        sa1 = mxg_gather(raw_a[1]);
        sb1 = mxg_gather(raw_b[1]);
      }
      if constexpr (MORE) {
        // the gathered values exist before their registers are loaded again
        asm volatile("" : : "v"(sa0), "v"(sb0));
        if constexpr (FMT == MXG_FP4) asm volatile("" : : "v"(sa1), "v"(sb1));
        sa_src += sa_step;
        sb_src += sb_step;
        mxg_load_scales<FMT, BL>(raw_a, raw_b, sa_src, sb_src, sa_off, sb_off, sa_stride,
                                 sb_stride);
      }
      // barrier 2: every wave's part of step k has landed
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const unsigned st = lds_base + (k & 1) * GP_STAGE_BYTES;
      unsigned b0[4], b1[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        b0[t] = st + b_at[BL == GP_NK ? 0 : t];
        b1[t] = st + b_at[BL == GP_NK ? 1 : t];
      }
      if constexpr (FMT == MXG_FP4) {
        MxgFrags4<BL> f0, f1;
        mxg_read_half4<BL, 0>(f0, st + a_at[0], b0);
        mxg_read_half4<BL, 1>(f1, st + a_at[1], b1);
        mxg_wait_half4<BL, true>(f0);  // chunk 1's reads stay in flight
        mxg_mma_half4<BL>(f0, acc, sa0, sb0);
        __builtin_amdgcn_sched_barrier(0);  // chunk 0's MFMAs stay above the wait
        mxg_wait_half4<BL, false>(f1);
        mxg_mma_half4<BL>(f1, acc, sa1, sb1);
      } else {
        MxgFrags8<BL> f;
        const unsigned a2[2] = {st + a_at[0], st + a_at[1]};
        mxg_read_step8<BL>(f, a2, b0, b1);
        mxg_wait_part8<BL, 0>(f);  // A tiles 2-3 stay in flight
        mxg_mma_part8<BL, 0>(f, acc, sa0, sb0);
        __builtin_amdgcn_sched_barrier(0);  // part 0's MFMAs stay above the wait
        mxg_wait_part8<BL, 1>(f);
        mxg_mma_part8<BL, 1>(f, acc, sa0, sb0);
      }
    };
    for (int k = 0; k + 1 < steps; k++) step(std::true_type{}, k);
    step(std::false_type{}, steps - 1);
    if (inject_here && round == inject_round) gp_inject(acc);
    gp_compare_round(acc, expected, wm, wn, lane, round, verdict);
  }
  if (store_c) gp_store_c(acc, C, N, m0, n0, wm, wn, lane);
  gp_store_record(records, wave, lane, place, verdict);
}

// The operand checks mx_gemm_pipe and mx6_gemm_pipe share: five 2-D tensors on
// one GPU, uint8 but expected; M, N and K from the packed rows of a_bits and
// b_bits per code (A [M, K a_bits/8]; B nk [N, ...], kn [K, N b_bits/8]); the
// scales' shapes. Leaves the scales contiguous. B's other dimension and the
// K step are the caller's to check.
struct MxgDims { long M, N, K; };
static MxgDims mxg_check_operands(const torch::Tensor& A, const torch::Tensor& B,
                                  torch::Tensor& scale_a, torch::Tensor& scale_b,
                                  const torch::Tensor& expected, int bl, long a_bits,
                                  long b_bits) {
  for (const torch::Tensor& t : {A, B, scale_a, scale_b, expected}) {
    TORCH_CHECK(t.is_cuda() && t.device() == A.device(),
                "A, B, the scales and expected must be on one GPU");
    TORCH_CHECK(t.dim() == 2, "A, B, the scales and expected must be 2-D");
  }
  TORCH_CHECK(A.dtype() == torch::kUInt8 && B.dtype() == torch::kUInt8 &&
                  scale_a.dtype() == torch::kUInt8 && scale_b.dtype() == torch::kUInt8,
              "A, B and the scales must be uint8");
  const long M = A.size(0), K = A.size(1) * 8 / a_bits;
  const long N = bl == GP_NK ? B.size(0) : B.size(1) * 8 / b_bits;
  // the kernel's per-lane offsets into a tile's rows are 32-bit
  TORCH_CHECK(M <= (1L << 22) && N <= (1L << 22) && K <= (1L << 22),
              "M, N and K must be <= 2^22");
  if (bl == GP_NK) {
    TORCH_CHECK(scale_b.sizes() == torch::IntArrayRef({N, K / 32}), "scale_b must be [", N, ",",
                K / 32, "]");
  } else {
    TORCH_CHECK(scale_b.sizes() == torch::IntArrayRef({K / 32, N}), "scale_b must be [", K / 32,
                ",", N, "]");
  }
  TORCH_CHECK(scale_a.sizes() == torch::IntArrayRef({M, K / 32}), "scale_a must be [", M, ",",
              K / 32, "]");
  scale_a = scale_a.contiguous();
  scale_b = scale_b.contiguous();
  return {M, N, K};
}

// fmt "mxfp8": e4m3, one code per byte; "mxfp4": e2m1, two codes per byte along
// K (A, B nk) or N (B kn), the even element in the low nibble. A [M,K]; B
// [N,K] ("nk") or [K,N] ("kn"); scale_a [M,K/32]; scale_b [N,K/32] or [K/32,N];
// all uint8, row-major. expected [128,128] fp32, the tile every workgroup must
// compute. One untimed warm-up launch, then one timed launch. Returns (records
// [grid*4,8] int32, C [M,N] fp32 when store_c else an empty tensor, elapsed_ms).
// The wrapper does not judge exactness: any finite operands give a correct GEMM.
std::tuple<torch::Tensor, torch::Tensor, double> mx_gemm_pipe(
    torch::Tensor A, torch::Tensor B, torch::Tensor scale_a, torch::Tensor scale_b,
    torch::Tensor expected, const std::string& fmt, const std::string& b_layout, long rounds,
    bool store_c, long inject_block, long inject_round) {
  const int f = fmt == "mxfp8" ? MXG_FP8 : fmt == "mxfp4" ? MXG_FP4 : -1;
  TORCH_CHECK(f >= 0, "fmt must be one of mxfp8, mxfp4; got ", fmt);
  const int bl = b_layout == "kn" ? GP_KN : b_layout == "nk" ? GP_NK : -1;
  TORCH_CHECK(bl >= 0, "b_layout must be one of kn, nk; got ", b_layout);
  const long bits = f == MXG_FP4 ? 4 : 8;
  const long BK = f == MXG_FP4 ? 256 : 128;
  const MxgDims d = mxg_check_operands(A, B, scale_a, scale_b, expected, bl, bits, bits);
  TORCH_CHECK(d.K >= BK && d.K % BK == 0, "K must be a positive multiple of ", BK, "; got ", d.K);
  if (bl == GP_NK) {
    TORCH_CHECK(B.size(1) * 8 == d.K * bits, "B must be [N,K] in ", d.K * bits / 8,
                " bytes per row");
  } else {
    TORCH_CHECK(B.size(0) == d.K, "B must be [K,N] with K=", d.K);
  }
  const GpRun run =
      gp_prepare(A, B, expected, d.M, d.N, d.K, rounds, store_c, inject_block, inject_round);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const double ms = warm_then_timed_ms(stream, [&]() {
    dispatch_int<4>(2 * f + bl, [&](auto case_c) {
      constexpr int c = decltype(case_c)::value;
      gp_launch(mx_gemm_pipe_kernel<c / 2, c % 2>, run, stream,
                static_cast<const char*>(A.data_ptr()), static_cast<const char*>(B.data_ptr()),
                scale_a.data_ptr<unsigned char>(), scale_b.data_ptr<unsigned char>());
    });
  });
  return std::make_tuple(run.records, run.C, ms);
}

// ---------------------------------------------------------------------------
// MX6 GEMM probe: mx_gemm_pipe's pipeline for the operands whose rows are not
// 128 bytes: MXFP6 (e2m3) and MXBF6 (e3m2), four codes in three bytes, and an
// MXFP8 A against MXFP6 or MXFP4 weights (W6A8, W4A8: cbsz != blgp).
// C = (A o scales).(B o scales) through v_mfma_scale_f32_16x16x128_f8f6f4.
//
// Kept as in mx_gemm_pipe_kernel, to be read side by side with it: 256 threads
// per 128x128 tile of C, waves 2x2, 4x4 MFMA tiles per wave, 64 accumulators
// held over the K loop; two LDS stages of 32 KiB (A region at 0, B region at
// 16 KiB); barrier 1 / issue step k+1 / wait / barrier 2 / read / MFMA; the
// scale bytes (one K chunk of four blocks per step: 4 A and 4 B
// global_load_ubyte per lane, mx6_load_scales) a step ahead, gathered into one VGPR per
// side and selected with op_sel; the last step peeled; verification, records,
// store_c and inject (gemm_pipe's helpers).
//
// New: a K step is 128 *elements* in every case, one scaled MFMA deep, so a
// side's tile of a step is 128 rows of 128 (8-bit), 96 (6-bit) or 64 (4-bit)
// bytes. A side is one of four kinds (AW, BW, BL choose them):
//
//   K8  8-bit, K-contiguous (A e4m3). As mx_gemm_pipe: 4 global_load_lds_dwordx4
//       per wave, two ds_read_b128 (chunks g and g+4: k = 16g.. and 64+16g..,
//       the 8-bit K walk), key (r>>1)&7.
//   K6  6-bit, K-contiguous (A, B nk). The tile is 768 16-byte chunks, 3 loads
//       per wave; chunk c lands at 16 c = row c/6, slot c%6, and fetches global
//       chunk slot ^ key(row) of the row's 96 bytes of this step. Lane (i, g)
//       holds k = 32g.., bits [6j, 6j+6) of six VGPRs: bytes 24g..24g+23 of
//       its row, the 8-byte units u = 3g, 3g+1, 3g+2 of the row's twelve, read
//       with three ds_read_b64 at 96 r + 16 ((u>>1) ^ key) + 8 (u&1): 8-byte
//       aligned, each inside one chunk.
//       key = (r>>3) & 1 (slots 0<->1, 2<->3, 4<->5). A row is 24 banks, so
//       the rows start on banks 24r mod 64 = 0, 24, 48, 8, 32, 56, 16, 40 and
//       rows r, r+8 on the same one. Assuming one LDS pass serves 32
//       consecutive lanes of a b64 read (groups g, g+1, 16 rows each, the same
//       read of each): with c0 = 2u mod 8, group g's rows 0-7 take banks
//       8m + c0 (+1), its rows 8-15, moved one slot = 4 banks by the key,
//       8m + c0 + 4 (+1); group g+1 wants unit u + 3, 6 banks on: 8m + c0 + 6
//       and 8m + c0 + 2. The four sets are disjoint and fill the 64 banks:
//       conflict degree 1 by construction under that assumption (2 without
//       the key); not measured with counters.
//   K4  4-bit, K-contiguous (B nk e2m1), 64-byte rows: 512 chunks, 2 loads per
//       wave, row c/4, slot c%4; lane (i, g) holds k = 32g.. = chunk g, one
//       ds_read_b128 at 64 r + 16 (g ^ key). Four rows fill the 64 banks, rows
//       r, r+4 start on the same one: key = (r>>2) & 3 puts the 16 rows of a
//       pass (16 lanes of a b128 read, as in gemm_pipe) on 16 different
//       4-bank spans: degree 1 by construction under that assumption.
//   T6  6-bit B kn: B [K, N 3/4], four codes of consecutive n in three bytes.
//       The fragment comes through ds_read_b96_tr_b6 (map: lds_tr_read above):
//       a group's 16 lanes address the k rows 32g + 16h + i for read h, lane i
//       the 12 bytes = 16 codes = one MFMA tile's columns of its row, and
//       receives column i, the lowest k in the lowest bits; the two reads are
//       the lane's 32 k in six VGPRs. The instruction is issued at 16-byte
//       aligned addresses only (what lds_tr_read enforces; less is not tried),
//       so the 12-byte units lie at a 16-byte pitch: a tile row (one k) is
//       eight units = 128 bytes, the tile 16 KiB.
//       They get there with global_load_lds_dword (lane l's dword lands at
//       M0 + 4 l, as the memory-path probe established): one instruction
//       fills two rows, lane l row l>>5, unit slot (l>>2)&7, word l&3; word 3
//       is the padding and fetches word 2 again, an address inside the tile
//       in any case. 16 instructions per wave and step. Chosen over a staged
//       global_load_dwordx3 / ds_write_b96 path because it keeps the pipeline
//       of the other kinds unchanged: no registers held over the MFMAs, no
//       lgkmcnt accounting for writes, one vmcnt wait. The direct dwordx3
//       form is not used: its lane-to-LDS map is not established here.
//       The dword loads move 16 KiB per step for 12 KiB of operands.
//       key = (k>>1) & 7 on the unit slot: a row is 32 banks, rows k, k+2
//       collide; the 16 rows of one read fall, per parity of k, on eight
//       different slots. Degree 1 by construction assuming one pass serves
//       the 16 lanes of a group, as for b128; if a pass serves 32 lanes, 96
//       banks are wanted and the degree is 2 at best. Not measured.
//       Row 2 (16 w + j) + (l>>5) of wave w's load j has key j & 7, a constant
//       per load: a lane keeps its row-and-word offset and its slot, and the
//       source unit slot ^ (j & 7) is one xor and one multiply-add per load.
//
// The 8-bit side walks K in two halves and the narrow side as 32g + j; the
// instruction pairs them by k, and lane group b's scale byte covers k in
// [32b, 32b+32) on both sides, so the scale loads do not depend on the kind.
//
// vmcnt, oldest first, with L = A loads + B loads per wave and step (K8 4, K6
// 3, K4 2, T6 16). Before the loop: LDS(0) [L], scales(0) [8]. Step k: after
// barrier 1, LDS(k+1) [L] is issued; in flight are LDS(k), scales(k),
// LDS(k+1), and s_waitcnt vmcnt(L) leaves exactly LDS(k+1): step k's operands
// have landed and its scale bytes are in registers. They are gathered, then
// scales(k+1) [8] is issued behind LDS(k+1). L = 7 for 8x6, 6 for 6x6 nk and
// 8x4, 19 for 6x6 kn; at most 2 L + 8 = 46 loads in flight, below the
// counter's 63. The last step waits vmcnt(0).
//
// lgkmcnt: B's four tiles and A tiles 0-1 are read, then A tiles 2-3 (R reads:
// K8 4, K6 6); lgkmcnt(R) before the 8 MFMAs of A tiles 0-1, lgkmcnt(0) before
// the other 8. The waits are followed by empty asm statements that name the
// fragment registers: volatile asm keeps its order, so no use moves above.
//
// Race and bounds: no wave waits for another workgroup; every loop bound is a
// launch argument; nothing is indexed by a loaded value; the wrapper fixes
// every shape the offsets are computed from; vector stores only. Build for
// gfx950: no scratch, 64 KiB of LDS (register counts in BENCHMARKS.md "MX6
// GEMM probe").
// ---------------------------------------------------------------------------
enum { MX6_K8 = 0, MX6_K6 = 1, MX6_K4 = 2, MX6_T6 = 3 };
constexpr int MX6_BK = 128;  // elements of K per step

template <int KIND> struct Mx6Side {  // K8, K6, K4
  static constexpr int ROW = KIND == MX6_K8 ? 128 : KIND == MX6_K6 ? 96 : 64;  // bytes in LDS
  static constexpr int CHUNKS = ROW / 16, LOADS = ROW / 32, OFFS = LOADS;
  static constexpr int READS = KIND == MX6_K8 ? 2 : KIND == MX6_K6 ? 3 : 1;  // per tile
};
template <> struct Mx6Side<MX6_T6> {
  static constexpr int ROW = 128, LOADS = 16, OFFS = 2, READS = 2;
};

template <int KIND> __device__ __forceinline__ int mx6_key(int r) {
  if constexpr (KIND == MX6_K6) return (r >> 3) & 1;
  else if constexpr (KIND == MX6_K4) return (r >> 2) & 3;
  else return (r >> 1) & 7;
}

// where this lane's bytes of each load come from, relative to the tile's first
// byte of the step; `pitch`: bytes from one row of the operand to the next
template <int KIND>
__device__ __forceinline__ void mx6_offsets(unsigned (&off)[Mx6Side<KIND>::OFFS], unsigned pitch,
                                            int wave, int lane) {
  typedef Mx6Side<KIND> S;
  if constexpr (KIND == MX6_T6) {
    off[0] = (unsigned)(lane >> 5) * pitch + 4 * min(lane & 3, 2);  // row and word
    off[1] = (lane >> 2) & 7;                                       // unit slot
  } else {
#pragma unroll
    for (int i = 0; i < S::LOADS; i++) {
      const int c = 64 * (wave * S::LOADS + i) + lane;
      const int r = c / S::CHUNKS, s = c % S::CHUNKS;
      off[i] = (unsigned)r * pitch + ((s ^ mx6_key<KIND>(r)) << 4);
    }
  }
}

// one side's direct-to-LDS loads of one wave for one K step into `region`
template <int KIND>
__device__ __forceinline__ void mx6_issue(const char* src,
                                          const unsigned (&off)[Mx6Side<KIND>::OFFS],
                                          unsigned pitch, GP_LDS_AS char* region, int wave) {
  typedef Mx6Side<KIND> S;
  if constexpr (KIND == MX6_T6) {
    // the eight source units slot ^ key are worked out again every step: held
    // over the K loop as 64-bit addresses they do not fit the register file
    unsigned slot = off[1];
    asm volatile("" : "+v"(slot));
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int pair = wave * 16 + j;                     // rows 2 pair, 2 pair + 1
      GP_LDS_AS char* to = region + pair * 256;           // wave-uniform: goes to M0
      const char* from = src + (size_t)(2 * pair) * pitch + (off[0] + 12 * (slot ^ (j & 7)));
      __builtin_amdgcn_global_load_lds((GP_GLOBAL_AS const unsigned*)from,
                                       (GP_LDS_AS unsigned*)to, 4, 0, 0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < S::LOADS; i++) {
      GP_LDS_AS char* to = region + (wave * S::LOADS + i) * 1024;
      __builtin_amdgcn_global_load_lds((GP_GLOBAL_AS const unsigned*)(src + off[i]),
                                       (GP_LDS_AS unsigned*)to, 16, 0, 0);
    }
  }
}

// LDS byte offsets, inside the side's region, of this lane's fragment reads:
// K kinds of tile 0 (tile t is 16 rows on, an immediate), T6 of each tile's
// first read (the second is 16 rows on). w: the wave's row (column) of the 2x2.
template <int KIND>
__device__ __forceinline__ void mx6_read_addrs(unsigned (&at)[4], int w, int i16, int g) {
  const int r = w * 64 + i16;
  at[0] = at[1] = at[2] = at[3] = 0;
  if constexpr (KIND == MX6_K8) {
    at[0] = r * 128 + ((g ^ mx6_key<KIND>(r)) << 4);
    at[1] = at[0] ^ 64;
  } else if constexpr (KIND == MX6_K6) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int u = 3 * g + j;
      at[j] = r * 96 + (((u >> 1) ^ mx6_key<KIND>(r)) << 4) + ((u & 1) << 3);
    }
  } else if constexpr (KIND == MX6_K4) {
    at[0] = r * 64 + ((g ^ mx6_key<KIND>(r)) << 4);
  } else {
    const int k = 32 * g + i16;
#pragma unroll
    for (int t = 0; t < 4; t++) at[t] = k * 128 + (((w * 4 + t) ^ mx6_key<KIND>(k)) << 4);
  }
}

// one 16-row tile's fragment of a side
template <int KIND> struct Mx6Frag;
template <> struct Mx6Frag<MX6_K8> { gp_i4 lo, hi; };
template <> struct Mx6Frag<MX6_K6> { gp_i2 p[3]; };
template <> struct Mx6Frag<MX6_K4> { gp_i4 q; };
template <> struct Mx6Frag<MX6_T6> { gp_i3 lo, hi; };

#define MX6_READ(INSN, DST, AT, OFF) \
  asm volatile(INSN " %0, %1 offset:%2" : "=v"(DST) : "v"(AT), "n"(OFF) : "memory")
// tile T of the side whose region starts REGION bytes into the stage; at:
// mx6_read_addrs plus the stage's LDS address
template <int KIND, int T, int REGION>
__device__ __forceinline__ void mx6_read_tile(Mx6Frag<KIND>& f, const unsigned (&at)[4]) {
  constexpr int O = REGION + T * 16 * Mx6Side<KIND>::ROW;
  if constexpr (KIND == MX6_K8) {
    MX6_READ("ds_read_b128", f.lo, at[0], O);
    MX6_READ("ds_read_b128", f.hi, at[1], O);
  } else if constexpr (KIND == MX6_K6) {
    MX6_READ("ds_read_b64", f.p[0], at[0], O);
    MX6_READ("ds_read_b64", f.p[1], at[1], O);
    MX6_READ("ds_read_b64", f.p[2], at[2], O);
  } else if constexpr (KIND == MX6_K4) {
    MX6_READ("ds_read_b128", f.q, at[0], O);
  } else {
    MX6_READ("ds_read_b96_tr_b6", f.lo, at[T], REGION);
    MX6_READ("ds_read_b96_tr_b6", f.hi, at[T], REGION + 2048);
  }
}
#undef MX6_READ
template <int KIND, int REGION>
__device__ __forceinline__ void mx6_read_pair(Mx6Frag<KIND>& f0, Mx6Frag<KIND>& f1,
                                              const unsigned (&at)[4],
                                              std::integral_constant<int, 0>) {
  mx6_read_tile<KIND, 0, REGION>(f0, at);
  mx6_read_tile<KIND, 1, REGION>(f1, at);
}
template <int KIND, int REGION>
__device__ __forceinline__ void mx6_read_pair(Mx6Frag<KIND>& f2, Mx6Frag<KIND>& f3,
                                              const unsigned (&at)[4],
                                              std::integral_constant<int, 1>) {
  mx6_read_tile<KIND, 2, REGION>(f2, at);
  mx6_read_tile<KIND, 3, REGION>(f3, at);
}
// after an s_waitcnt: the fragment's registers are valid from here on
template <int KIND> __device__ __forceinline__ void mx6_hold(Mx6Frag<KIND>& f) {
  if constexpr (KIND == MX6_K8) asm volatile("" : "+v"(f.lo), "+v"(f.hi));
  else if constexpr (KIND == MX6_K6) asm volatile("" : "+v"(f.p[0]), "+v"(f.p[1]), "+v"(f.p[2]));
  else if constexpr (KIND == MX6_K4) asm volatile("" : "+v"(f.q));
  else asm volatile("" : "+v"(f.lo), "+v"(f.hi));
}
// the MFMA's operand; the 6- and 4-bit forms read VGPRs 0-5 and 0-3 only
template <int KIND> __device__ __forceinline__ i32x8 mx6_operand(const Mx6Frag<KIND>& f) {
  if constexpr (KIND == MX6_K8) {
    return __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7);
  } else if constexpr (KIND == MX6_K6) {
    return (i32x8){f.p[0][0], f.p[0][1], f.p[1][0], f.p[1][1], f.p[2][0], f.p[2][1], 0, 0};
  } else if constexpr (KIND == MX6_K4) {
    return (i32x8){f.q[0], f.q[1], f.q[2], f.q[3], 0, 0, 0, 0};
  } else {
    return (i32x8){f.lo[0], f.lo[1], f.lo[2], f.hi[0], f.hi[1], f.hi[2], 0, 0};
  }
}

// the step's vmcnt wait; names the scale registers it makes valid. CNT: the
// direct loads of step k+1, issued after them, that stay in flight
template <int CNT>
__device__ __forceinline__ void mx6_wait_vm(unsigned (&ra)[2][4], unsigned (&rb)[2][4]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[0][2]), "+v"(ra[0][3]),
                 "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3])
               : "n"(CNT)
               : "memory");
}

// The lane's eight scale loads of one step, the addresses of mxg_load_scales'
// one K chunk (A, B nk: tile t is `stride` bytes on; B kn: 16 columns on), as
// one asm statement. mxg_load_scales issues one statement per load; where the
// compiler reloads a base address from an SGPR it spilled to a VGPR lane
// (v_readlane) right in front of such a statement, the five wait states a
// VMEM instruction needs after a VALU write of an SGPR it reads are missing:
// the hazard recognizer does not look into inline assembly, and the kn
// instantiation has that register pressure (seen on an MI355X as scale bytes
// of A tiles 2-3 from a stale address). Here every base is an input of the
// one statement, so all reloads come before it, and it opens with the wait
// states.
template <int BL>
__device__ __forceinline__ void mx6_load_scales(unsigned (&ra)[2][4], unsigned (&rb)[2][4],
                                                const unsigned char* sa, const unsigned char* sb,
                                                unsigned a_off, unsigned b_off, size_t a_stride,
                                                size_t b_stride) {
  const unsigned char* sa1 = sa + a_stride;
  const unsigned char* sa2 = sa1 + a_stride;
  const unsigned char* sa3 = sa2 + a_stride;
  if constexpr (BL == GP_NK) {
    const unsigned char* sb1 = sb + b_stride;
    const unsigned char* sb2 = sb1 + b_stride;
    const unsigned char* sb3 = sb2 + b_stride;
    asm volatile("s_nop 4\n\t"
                 "global_load_ubyte %0, %8, %10\n\t"
                 "global_load_ubyte %1, %8, %11\n\t"
                 "global_load_ubyte %2, %8, %12\n\t"
                 "global_load_ubyte %3, %8, %13\n\t"
                 "global_load_ubyte %4, %9, %14\n\t"
                 "global_load_ubyte %5, %9, %15\n\t"
                 "global_load_ubyte %6, %9, %16\n\t"
                 "global_load_ubyte %7, %9, %17"
                 : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[0][2]), "+v"(ra[0][3]),
                   "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3])
                 : "v"(a_off), "v"(b_off), "s"(sa), "s"(sa1), "s"(sa2), "s"(sa3), "s"(sb),
                   "s"(sb1), "s"(sb2), "s"(sb3)
                 : "memory");
  } else {
    asm volatile("s_nop 4\n\t"
                 "global_load_ubyte %0, %8, %10\n\t"
                 "global_load_ubyte %1, %8, %11\n\t"
                 "global_load_ubyte %2, %8, %12\n\t"
                 "global_load_ubyte %3, %8, %13\n\t"
                 "global_load_ubyte %4, %9, %14\n\t"
                 "global_load_ubyte %5, %9, %14 offset:16\n\t"
                 "global_load_ubyte %6, %9, %14 offset:32\n\t"
                 "global_load_ubyte %7, %9, %14 offset:48"
                 : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[0][2]), "+v"(ra[0][3]),
                   "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[0][2]), "+v"(rb[0][3])
                 : "v"(a_off), "v"(b_off), "s"(sa), "s"(sa1), "s"(sa2), "s"(sa3), "s"(sb)
                 : "memory");
  }
}

// op_sel must be an immediate
#define MX6_MMA(I, J)                                                                       \
  acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[I], b[J], acc[I][J], FA, FB, \
                                                               I, sa, J, sb)
#define MX6_MMA_ROW(I) MX6_MMA(I, 0); MX6_MMA(I, 1); MX6_MMA(I, 2); MX6_MMA(I, 3)

template <int AW, int BW, int BL, int FA, int FB>
__global__ void __launch_bounds__(256, 2)
mx6_gemm_pipe_kernel(const char* __restrict__ A, const char* __restrict__ B,
                     const unsigned char* __restrict__ scale_a,
                     const unsigned char* __restrict__ scale_b, const float* __restrict__ expected,
                     int4* __restrict__ records, float* __restrict__ C, int N, int K, int tiles_n,
                     int rounds, int store_c, int inject_block, int inject_round) {
  static_assert((AW == 8 || AW == 6) && (BW == 6 || BW == 4) && (BL == GP_NK || (AW == 6 && BW == 6)),
                "instantiated: 6x6 nk and kn, 8x6 nk, 8x4 nk");
  __shared__ __attribute__((aligned(1024))) char mx6_lds[GP_STAGES * GP_STAGE_BYTES];
  constexpr int AK = AW == 8 ? MX6_K8 : MX6_K6;
  constexpr int BKIND = BL == GP_KN ? MX6_T6 : BW == 6 ? MX6_K6 : MX6_K4;
  typedef Mx6Side<AK> SA;
  typedef Mx6Side<BKIND> SB;
  constexpr int STEP_BLOCKS = MX6_BK / 32;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int i16 = lane & 15, g = lane >> 4;
  const int m0 = (blockIdx.x / tiles_n) * GP_TILE, n0 = (blockIdx.x % tiles_n) * GP_TILE;
  const unsigned place = hw_word();
  const int steps = K / MX6_BK;
  // bytes from one row to the next: A [M,K], B nk [N,K], B kn [K,N]
  const unsigned a_pitch = ((unsigned)K >> 3) * AW;
  const unsigned b_pitch = ((unsigned)(BL == GP_NK ? K : N) >> 3) * BW;
  const unsigned kblocks = (unsigned)K >> 5;

  unsigned aoff[SA::OFFS], boff[SB::OFFS];
  mx6_offsets<AK>(aoff, a_pitch, wave, lane);
  mx6_offsets<BKIND>(boff, b_pitch, wave, lane);
  const char* a_tile = A + (size_t)m0 * a_pitch;
  const char* b_tile = BL == GP_NK ? B + (size_t)n0 * b_pitch : B + (n0 >> 3) * BW;
  const size_t a_step = MX6_BK / 8 * AW;
  const size_t b_step = BL == GP_NK ? (size_t)(MX6_BK / 8 * BW) : (size_t)MX6_BK * b_pitch;

  // the lane's scale bytes of a step, as in mx_gemm_pipe_kernel
  const unsigned sa_off = (unsigned)(wm * 64 + i16) * kblocks + g;
  const unsigned sb_off = BL == GP_NK ? (unsigned)(wn * 64 + i16) * kblocks + g
                                      : (unsigned)g * (unsigned)N + wn * 64 + i16;
  const size_t sa_stride = (size_t)16 * kblocks;
  const size_t sb_stride = BL == GP_NK ? (size_t)16 * kblocks : (size_t)4 * N;
  const unsigned char* sa_tile = scale_a + (size_t)m0 * kblocks;
  const unsigned char* sb_tile = BL == GP_NK ? scale_b + (size_t)n0 * kblocks : scale_b + n0;
  const size_t sa_step = STEP_BLOCKS;
  const size_t sb_step = BL == GP_NK ? (size_t)STEP_BLOCKS : (size_t)STEP_BLOCKS * N;

  unsigned a_at[4], b_at[4];
  mx6_read_addrs<AK>(a_at, wm, i16, g);
  mx6_read_addrs<BKIND>(b_at, wn, i16, g);

  GP_LDS_AS char* lds = (GP_LDS_AS char*)mx6_lds;
  const unsigned lds_base = (unsigned)reinterpret_cast<__UINTPTR_TYPE__>(lds);
  const bool inject_here = (int)blockIdx.x == inject_block && threadIdx.x == 0;
  GpVerdict verdict;
  unsigned raw_a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, raw_b[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  f32x4 acc[4][4];
  for (int round = 0; round < rounds; round++) {
    GP_ZERO_ACC(acc)
    const char* a_src = a_tile;
    const char* b_src = b_tile;
    const unsigned char* sa_src = sa_tile;
    const unsigned char* sb_src = sb_tile;
    // stage 0 may still be read by a wave that is finishing the last round
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    mx6_issue<AK>(a_src, aoff, a_pitch, lds, wave);
    mx6_issue<BKIND>(b_src, boff, b_pitch, lds + GP_TILE_BYTES, wave);
    mx6_load_scales<BL>(raw_a, raw_b, sa_src, sb_src, sa_off, sb_off, sa_stride, sb_stride);
    // one K step; the last one is peeled, for the reason mx_gemm_pipe_kernel gives
    auto step = [&](auto more_c, int k) {
      constexpr bool MORE = decltype(more_c)::value;
      // barrier 1: the other stage has been read for the last time
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if constexpr (MORE) {
        a_src += a_step;
        b_src += b_step;
        GP_LDS_AS char* next = lds + ((k + 1) & 1) * GP_STAGE_BYTES;
        mx6_issue<AK>(a_src, aoff, a_pitch, next, wave);
        mx6_issue<BKIND>(b_src, boff, b_pitch, next + GP_TILE_BYTES, wave);
      }
      // step k's operands and scales are in; step k+1's direct loads stay in flight
      mx6_wait_vm<MORE ? SA::LOADS + SB::LOADS : 0>(raw_a, raw_b);
      const int sa = mxg_gather(raw_a[0]), sb = mxg_gather(raw_b[0]);
      if constexpr (MORE) {
        // the gathered values exist before their registers are loaded again
        asm volatile("" : : "v"(sa), "v"(sb));
        sa_src += sa_step;
        sb_src += sb_step;
        mx6_load_scales<BL>(raw_a, raw_b, sa_src, sb_src, sa_off, sb_off, sa_stride, sb_stride);
      }
      // barrier 2: every wave's part of step k has landed
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const unsigned st = lds_base + (k & 1) * GP_STAGE_BYTES;
      unsigned aa[4], bb[4];
#pragma unroll
      for (int t = 0; t < 4; t++) {
        aa[t] = st + a_at[t];
        bb[t] = st + b_at[t];
      }
      Mx6Frag<AK> fa[4];
      Mx6Frag<BKIND> fb[4];
      mx6_read_pair<BKIND, GP_TILE_BYTES>(fb[0], fb[1], bb, std::integral_constant<int, 0>{});
      mx6_read_pair<BKIND, GP_TILE_BYTES>(fb[2], fb[3], bb, std::integral_constant<int, 1>{});
      mx6_read_pair<AK, 0>(fa[0], fa[1], aa, std::integral_constant<int, 0>{});
      mx6_read_pair<AK, 0>(fa[2], fa[3], aa, std::integral_constant<int, 1>{});
      i32x8 a[4], b[4];
      // A tiles 2-3 stay in flight
      asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(2 * SA::READS) : "memory");
#pragma unroll
      for (int t = 0; t < 4; t++) {
        mx6_hold<BKIND>(fb[t]);
        b[t] = mx6_operand<BKIND>(fb[t]);
      }
      mx6_hold<AK>(fa[0]);
      mx6_hold<AK>(fa[1]);
      a[0] = mx6_operand<AK>(fa[0]);
      a[1] = mx6_operand<AK>(fa[1]);
      MX6_MMA_ROW(0);
      MX6_MMA_ROW(1);
      __builtin_amdgcn_sched_barrier(0);  // these MFMAs stay above the wait
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mx6_hold<AK>(fa[2]);
      mx6_hold<AK>(fa[3]);
      a[2] = mx6_operand<AK>(fa[2]);
      a[3] = mx6_operand<AK>(fa[3]);
      MX6_MMA_ROW(2);
      MX6_MMA_ROW(3);
    };
    for (int k = 0; k + 1 < steps; k++) step(std::true_type{}, k);
    step(std::false_type{}, steps - 1);
    if (inject_here && round == inject_round) gp_inject(acc);
    gp_compare_round(acc, expected, wm, wn, lane, round, verdict);
  }
  if (store_c) gp_store_c(acc, C, N, m0, n0, wm, wn, lane);
  gp_store_record(records, wave, lane, place, verdict);
}
#undef MX6_MMA_ROW
#undef MX6_MMA
#undef GP_ZERO_ACC

// the instantiated cases: operand formats by name, bits per code, the
// instruction's format code
struct Mx6Format { const char* name; int bits, code; };
static const Mx6Format MX6_FORMATS[4] = {
    {"mxfp8", 8, 0}, {"mxfp6", 6, 2}, {"mxbf6", 6, 3}, {"mxfp4", 4, 4}};
constexpr int MX6_CASES = 6;
// (a format, b format, b layout) as indices into MX6_FORMATS and GP_KN / GP_NK
static const int MX6_CASE[MX6_CASES][3] = {{1, 1, GP_NK}, {1, 1, GP_KN}, {2, 2, GP_NK},
                                           {2, 2, GP_KN}, {0, 1, GP_NK}, {0, 3, GP_NK}};

// a_fmt / b_fmt "mxfp8" (e4m3, one code per byte), "mxfp6" (e2m3) and "mxbf6"
// (e3m2: four codes in three bytes, a little-endian bit stream), "mxfp4" (e2m1,
// the even element in the low nibble); the pairs and layouts of MX6_CASE. A
// [M, K bits/8]; B [N, K bits/8] ("nk") or [K, N 3/4] ("kn", 6-bit); scale_a
// [M,K/32]; scale_b [N,K/32] or [K/32,N]; all uint8, row-major. expected
// [128,128] fp32. One untimed warm-up launch, then one timed launch. Returns
// (records [grid*4,8] int32, C [M,N] fp32 when store_c else empty, elapsed_ms).
std::tuple<torch::Tensor, torch::Tensor, double> mx6_gemm_pipe(
    torch::Tensor A, torch::Tensor B, torch::Tensor scale_a, torch::Tensor scale_b,
    torch::Tensor expected, const std::string& a_fmt, const std::string& b_fmt,
    const std::string& b_layout, long rounds, bool store_c, long inject_block,
    long inject_round) {
  int fa = -1, fb = -1;
  for (int f = 0; f < 4; f++) {
    if (a_fmt == MX6_FORMATS[f].name) fa = f;
    if (b_fmt == MX6_FORMATS[f].name) fb = f;
  }
  TORCH_CHECK(fa >= 0 && fb >= 0, "a_fmt and b_fmt must be among mxfp8, mxfp6, mxbf6, mxfp4; got ",
              a_fmt, ", ", b_fmt);
  const int bl = b_layout == "kn" ? GP_KN : b_layout == "nk" ? GP_NK : -1;
  TORCH_CHECK(bl >= 0, "b_layout must be one of kn, nk; got ", b_layout);
  int which = -1;
  for (int c = 0; c < MX6_CASES; c++)
    if (MX6_CASE[c][0] == fa && MX6_CASE[c][1] == fb && MX6_CASE[c][2] == bl) which = c;
  TORCH_CHECK(which >= 0, "unsupported case ", a_fmt, " x ", b_fmt, " ", b_layout,
              ": mxfp6 and mxbf6 with themselves (nk, kn), mxfp8 x mxfp6 and mxfp8 x mxfp4 (nk)");
  const long abits = MX6_FORMATS[fa].bits, bbits = MX6_FORMATS[fb].bits;
  const MxgDims d = mxg_check_operands(A, B, scale_a, scale_b, expected, bl, abits, bbits);
  TORCH_CHECK(d.K * abits == A.size(1) * 8, "A's ", A.size(1),
              " bytes per row hold no whole number of ", abits, "-bit codes");
  TORCH_CHECK(d.K >= MX6_BK && d.K % MX6_BK == 0, "K must be a positive multiple of 128; got ",
              d.K);
  if (bl == GP_NK) {
    TORCH_CHECK(B.size(1) * 8 == d.K * bbits, "B must be [N,K] in ", d.K * bbits / 8,
                " bytes per row");
  } else {
    TORCH_CHECK(B.size(0) == d.K && B.size(1) * 8 == d.N * bbits, "B must be [K,N] with K=", d.K,
                " in ", d.N * bbits / 8, " bytes per row");
  }
  const GpRun run =
      gp_prepare(A, B, expected, d.M, d.N, d.K, rounds, store_c, inject_block, inject_round);
  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto kernel) {
    gp_launch(kernel, run, stream, static_cast<const char*>(A.data_ptr()),
              static_cast<const char*>(B.data_ptr()), scale_a.data_ptr<unsigned char>(),
              scale_b.data_ptr<unsigned char>());
  };
  const double ms = warm_then_timed_ms(stream, [&]() {
    switch (which) {  // the order of MX6_CASE
      case 0: launch(mx6_gemm_pipe_kernel<6, 6, GP_NK, 2, 2>); break;
      case 1: launch(mx6_gemm_pipe_kernel<6, 6, GP_KN, 2, 2>); break;
      case 2: launch(mx6_gemm_pipe_kernel<6, 6, GP_NK, 3, 3>); break;
      case 3: launch(mx6_gemm_pipe_kernel<6, 6, GP_KN, 3, 3>); break;
      case 4: launch(mx6_gemm_pipe_kernel<8, 6, GP_NK, 0, 2>); break;
      default: launch(mx6_gemm_pipe_kernel<8, 4, GP_NK, 0, 4>); break;
    }
  });
  return std::make_tuple(run.records, run.C, ms);
}

py::dict device_info(int dev) {
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, dev));
  py::dict d;
  d["name"] = std::string(prop.name);
  d["gcnArchName"] = std::string(prop.gcnArchName);
  d["multiProcessorCount"] = prop.multiProcessorCount;
  d["totalGlobalMem"] = (long long)prop.totalGlobalMem;
  d["clockRate_kHz"] = prop.clockRate;
  d["warpSize"] = prop.warpSize;
  return d;
}

int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return 0;
  return n;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X GPU health-probe kernels (gfx950 HIP)";
  // default geometry from an on-hardware sweep (profiles/interference_r01.md):
  // 32768x1024 sustains 5.6 TB/s vs 5.0-5.2 at 8192x256 (+10%)
  m.def("hbm_triad_gbps", &hbm_triad_gbps, py::arg("size_mb") = 1024, py::arg("iters") = 10,
        py::arg("blocks") = 32768, py::arg("threads") = 1024,
        "Streaming HBM bandwidth in GB/s (triad: 2 reads + 1 write)");
  m.def("mfma_check", &mfma_check, py::arg("A"), py::arg("B"), py::arg("blocks") = 2048,
        py::arg("repeats") = 1, "Per-wave bf16 MFMA tile GEMM across all CUs");
  m.def("mfma_check_fp8", &mfma_check_fp8, py::arg("A"), py::arg("B"), py::arg("blocks") = 2048,
        "Per-wave fp8 (OCP e4m3) MFMA tile GEMM across all CUs");
  m.def("mfma_check_mx", &mfma_check_mx, py::arg("A"), py::arg("B"), py::arg("blocks") = 2048,
        py::arg("fmt") = 0, py::arg("scale_a") = 127, py::arg("scale_b") = 127,
        "Per-wave MX block-scaled MFMA (16x16x128 f8f6f4) tile; fmt 0=fp8, 4=fp4; "
        "scale_a/scale_b: one uniform e8m0 byte per operand");
  m.def("mfma_burn", &mfma_burn, py::arg("A"), py::arg("B"), py::arg("expected"), py::arg("fmt"),
        py::arg("blocks") = 2048, py::arg("chain") = 1024, py::arg("rounds") = 64,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1,
        "Sustained MFMA burn-in (fmt bf16|fp8|mx8|mx4): rounds x chain dependent MFMAs on 4 "
        "accumulators per wave, verified bitwise; returns (per-wave records [waves,4], ms)");
  m.def("mx_scale_tile", &mx_scale_tile, py::arg("A"), py::arg("B"), py::arg("scale_a"),
        py::arg("scale_b"), py::arg("fmt_a"), py::arg("fmt_b"), py::arg("shape"),
        py::arg("sel_a") = 0, py::arg("sel_b") = 0, py::arg("blocks") = 2048,
        "Per-wave MX block-scaled MFMA tile with per-lane E8M0 scales: formats 0 e4m3, 1 e5m2, "
        "2 e2m3, 3 e3m2, 4 e2m1 (one code per byte), shape 0 = 16x16x128, 1 = 32x32x64, "
        "sel_a/sel_b the scale byte each side reads; returns [waves, M, M] fp32");
  m.def("mx_scale_burn", &mx_scale_burn, py::arg("A"), py::arg("B"), py::arg("scale_a"),
        py::arg("scale_b"), py::arg("expected"), py::arg("fmt"), py::arg("shape"),
        py::arg("blocks") = 2048, py::arg("chain") = 128, py::arg("rounds") = 256,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1,
        "Sustained MX block-scaled MFMA burn (fmt 0|2|4, shape 0|1) with per-lane scales and the "
        "scale byte select rotating every step, verified bitwise; returns (per-wave records "
        "[waves,4], ms)");
  m.def("matrix_tile", &matrix_tile, py::arg("path"), py::arg("A"), py::arg("B"),
        py::arg("blocks") = 2048, py::arg("index") = py::none(), py::arg("abid") = 0,
        "Per-wave tile of one matrix path (f64, f32, f16, bf16, i8, fp8/bf8 MFMA shapes and the "
        "2:4 sparse smfmac forms, named as in ops.MATRIX_PATHS); sparse paths take A compressed "
        "with `index` (positions 0..3) and the index part select `abid`; returns [waves, M, M] "
        "in the accumulator's type");
  m.def("matrix_burn", &matrix_burn, py::arg("path"), py::arg("A"), py::arg("B"),
        py::arg("expected"), py::arg("blocks") = 2048, py::arg("chain") = 256,
        py::arg("rounds") = 64, py::arg("inject_wave") = -1, py::arg("inject_round") = -1,
        py::arg("index") = py::none(), py::arg("abid") = 0,
        "Sustained burn of one matrix path: rounds x chain dependent MFMAs on 4 accumulators per "
        "wave, verified bitwise; returns (per-wave records [waves,4], ms)");
  m.def("p2p_gbps", &p2p_gbps, py::arg("src_dev"), py::arg("dst_dev"), py::arg("size_mb") = 256,
        py::arg("iters") = 10, "xGMI peer-to-peer copy bandwidth in GB/s");
  m.def("hbm_sweep", &hbm_sweep, py::arg("max_gib") = 16, py::arg("chunk_gib") = 4,
        py::arg("seed") = 1,
        "Stuck-bit pattern sweep over up to max_gib GiB of HBM; returns error count");
  m.def("hbm_march", &hbm_march, py::arg("max_bytes") = 16L << 30,
        py::arg("chunk_bytes") = 4L << 30, py::arg("seed") = 1, py::arg("blocks") = 2048,
        py::arg("max_log") = 64, py::arg("inject_index") = -1, py::arg("inject_pass") = -1,
        py::arg("inject_bit") = 0,
        "HBM march: write/verify in both polarities, 16 B per lane, sweep-unique pattern, each "
        "launch timed; returns per-workgroup records [launches,blocks,16], a bad-location log "
        "and the bytes tested");
  m.def("lds_check", &lds_check, py::arg("blocks") = 2048, py::arg("seed") = 1,
        "LDS slab write/read-verify across the chip; returns error count");
  m.def("lds_march", &lds_march, py::arg("blocks"), py::arg("rounds"), py::arg("seed"),
        py::arg("inject_block") = -1, py::arg("inject_word") = -1, py::arg("inject_pass") = -1,
        py::arg("inject_bit") = 0,
        "Full-LDS (160 KiB per CU) march: both polarities, b32 and b128 read-back, timed; "
        "returns (per-wave records [blocks*4,8], ms)");
  m.def("valu_burn", &valu_burn, py::arg("expected"), py::arg("section"), py::arg("seed") = 1,
        py::arg("blocks") = 2048, py::arg("chain") = 1024, py::arg("rounds") = 33,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1, py::arg("inject_lane") = -1,
        py::arg("inject_bit") = -1,
        "Sustained VALU burn (section int|f32|f64|xlane|trans): rounds x chain dependent steps "
        "per lane, verified bitwise against expected; returns (per-wave records [waves,8], ms)");
  m.def("vgpr_march", &vgpr_march, py::arg("blocks"), py::arg("rounds"), py::arg("seed"),
        py::arg("inject_wave") = -1, py::arg("inject_target") = 0, py::arg("inject_lane") = 0,
        py::arg("inject_bit") = 0, py::arg("inject_pass") = -1,
        "Register-file march (480 of the 512 VGPR+AGPR entries per lane of every SIMD): both "
        "polarities, timed; returns (per-wave records [blocks*4,8], ms, workgroups per CU)");
  m.def("salu_burn", &salu_burn, py::arg("expected"), py::arg("section"), py::arg("seed") = 1,
        py::arg("blocks") = 2048, py::arg("chain") = 64, py::arg("rounds") = 33,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1, py::arg("inject_chain") = -1,
        py::arg("inject_bit") = -1,
        "Sustained scalar-ALU burn (section s32|s64|ctl|mask): rounds x chain dependent steps on "
        "eight states per wave (64 lanes for mask), verified bitwise against expected; returns "
        "(per-wave records [waves,8], ms)");
  m.def("sgpr_march", &sgpr_march, py::arg("blocks"), py::arg("rounds"), py::arg("seed"),
        py::arg("inject_wave") = -1, py::arg("inject_bit") = 0, py::arg("inject_pass") = -1,
        "SGPR march (s32..s101 of every wave): both polarities, timed; returns (per-wave records "
        "[blocks*4,8], ms, waves per SIMD by the occupancy query)");
  m.def("scalar_load_check", &scalar_load_check, py::arg("pattern"), py::arg("seed"),
        py::arg("blocks"), py::arg("rounds"),
        "Scalar-load check: every wave reads pattern [2,W] with s_load_dword, x2, x4, x8 and x16 "
        "and compares on the SALU; returns (per-wave records [blocks*4,8], ms)");
  m.def("atomic_burn", &atomic_burn, py::arg("expected"), py::arg("section"), py::arg("seed") = 1,
        py::arg("blocks") = 2048, py::arg("chain") = 8, py::arg("rounds") = 33,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1, py::arg("inject_lane") = -1,
        py::arg("inject_bit") = -1,
        "Exact atomic burn (section g32|g64|gfp|lds): rounds x chain steps of returning and "
        "non-returning atomics on cells each lane owns, every returned value and the final cells "
        "verified bitwise; returns (per-wave records [waves,8], ms)");
  m.def("atomic_contend", &atomic_contend, py::arg("section"), py::arg("seed"), py::arg("blocks"),
        py::arg("per_lane"), py::arg("cells"),
        "Contended atomics (section ticket|reduce|cas) from every workgroup on `cells` shared "
        "cells 4 KiB apart; returns {shared, owner, records, ms} for the host to judge");
  m.def("mempath_probe", &mempath_probe, py::arg("section"), py::arg("blocks"), py::arg("rounds"),
        py::arg("seed"), py::arg("inject_block") = -1, py::arg("inject_step") = -1,
        py::arg("inject_offset") = -1, py::arg("inject_bit") = 0,
        "Memory-path probe (section buf|oob|lds|forms): buffer addressing in every width, the "
        "descriptor's bounds check, direct-to-LDS loads, sub-dword, d16 and wide forms, verified "
        "bitwise; returns (per-wave records [blocks*4,8], ms)");
  m.def("cvt_sweep", &cvt_sweep, py::arg("path"), py::arg("inputs"), py::arg("scales"),
        py::arg("expected"), py::arg("blocks") = 2048, py::arg("seed") = 1,
        "Conversion sweep of one path (ops.CVT_PATHS): every wave walks the whole operand table "
        "out of LDS through one fp8/fp6/fp4/bf16 convert form, every select, compared bitwise "
        "(stochastic-rounding paths: against the two bracket codes); returns (per-wave records "
        "[blocks*4,8], ms)");
  m.def("cvt_burn", &cvt_burn, py::arg("section"), py::arg("expected"), py::arg("seed") = 1,
        py::arg("blocks") = 2048, py::arg("chain") = 1024, py::arg("rounds") = 33,
        py::arg("inject_wave") = -1, py::arg("inject_round") = -1, py::arg("inject_lane") = -1,
        py::arg("inject_bit") = -1,
        "Sustained conversion burn (section fp8|bf8|fp6|fp4|bf16): rounds x chain dependent "
        "encode-decode steps per lane, verified bitwise against expected; returns (per-wave "
        "records [waves,8], ms)");
  m.def("lds_tr_read", &lds_tr_read, py::arg("width"), py::arg("image"), py::arg("addrs"),
        "One LDS transpose read (ds_read_b64_tr_b16/b8/b4, ds_read_b96_tr_b6 for width 16/8/4/6) "
        "per lane at addrs[lane] into the image; returns the result registers [64,2] ([64,3])");
  m.def("gemm_pipe", &gemm_pipe, py::arg("A"), py::arg("B"), py::arg("expected"), py::arg("fmt"),
        py::arg("b_layout"), py::arg("rounds") = 1, py::arg("store_c") = false,
        py::arg("inject_block") = -1, py::arg("inject_round") = -1,
        "Tiled GEMM pipeline (fmt bf16|fp8, b_layout kn|nk): direct-to-LDS loads, LDS fragment "
        "reads (transpose reads for kn) and MFMAs, every 128x128 tile compared bitwise with "
        "expected each round; returns (per-wave records [grid*4,8], C or empty, ms)");
  m.def("mx_gemm_pipe", &mx_gemm_pipe, py::arg("A"), py::arg("B"), py::arg("scale_a"),
        py::arg("scale_b"), py::arg("expected"), py::arg("fmt"), py::arg("b_layout"),
        py::arg("rounds") = 1, py::arg("store_c") = false, py::arg("inject_block") = -1,
        py::arg("inject_round") = -1,
        "Block-scaled tiled GEMM pipeline (fmt mxfp8|mxfp4, b_layout kn|nk): direct-to-LDS loads, "
        "LDS fragment reads (8- and 4-bit transpose reads for kn), per-block E8M0 scales streamed "
        "from memory and the scaled 16x16x128 MFMA, every 128x128 tile compared bitwise with "
        "expected each round; returns (per-wave records [grid*4,8], C or empty, ms)");
  m.def("mx6_gemm_pipe", &mx6_gemm_pipe, py::arg("A"), py::arg("B"), py::arg("scale_a"),
        py::arg("scale_b"), py::arg("expected"), py::arg("a_fmt"), py::arg("b_fmt"),
        py::arg("b_layout"), py::arg("rounds") = 1, py::arg("store_c") = false,
        py::arg("inject_block") = -1, py::arg("inject_round") = -1,
        "Block-scaled tiled GEMM pipeline for 6-bit and mixed-width operands (mxfp6 / mxbf6 with "
        "themselves, nk and kn; mxfp8 x mxfp6 and mxfp8 x mxfp4, nk): 96- and 64-byte rows through "
        "direct-to-LDS loads, ds_read_b64 / ds_read_b96_tr_b6 fragments, streamed E8M0 scales and "
        "the scaled 16x16x128 MFMA, every 128x128 tile compared bitwise with expected each round; "
        "returns (per-wave records [grid*4,8], C or empty, ms)");
  m.def("cu_coverage", &cu_coverage, py::arg("blocks") = 4096,
        "Per-wave (XCC_ID<<16 | HW_ID) placement words for CU-coverage checks");
  m.def("device_info", &device_info, py::arg("dev") = 0);
  m.def("device_count", &device_count);
}
