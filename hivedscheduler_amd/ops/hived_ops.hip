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
//  - p2p copy:   xGMI link bandwidth between two GPUs (expected ~153 GB/s per
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
  m.def("cu_coverage", &cu_coverage, py::arg("blocks") = 4096,
        "Per-wave (XCC_ID<<16 | HW_ID) placement words for CU-coverage checks");
  m.def("device_info", &device_info, py::arg("dev") = 0);
  m.def("device_count", &device_count);
}
