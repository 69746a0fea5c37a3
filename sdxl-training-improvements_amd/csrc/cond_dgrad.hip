// Conditioning gradients (d prompt_embeds, d pooled): the input-gradient product of the hoisted K | V projections and of
// add_embedding.linear_1, in fp32.
//
//   C32[M][N] (ldc) = sum_g A_g[M][K_g] (lda_g, bf16) . W_g[K_g][N] (ldb_g, bf16),   g <= 2 groups, fp32 accumulate, fp32 out
//
// M is small and ragged (B * 77; B for the pooled slice), the reduction long (12 800 + 153 600 at SDXL-base): the product is bound by the
// weight stream.  One workgroup (4 waves) owns ALL rows of a 128-column strip up to M = 320 (row tile 64 * RT, RT = 1 .. 5 by M), so the
// weight crosses HBM once; the reduction is cut into (group, K-chunk) pieces over blockIdx.z so that the grid fills the chip, every piece
// writes its fp32 partial tile into a slab with plain stores, and a second kernel adds the pieces of an element in ascending piece order.
// No atomics: the result depends on the shapes only and is bitwise reproducible.
// The step's gradient gate (out[7] of the loss) is already a factor of dK | dV and dA1 and is not applied again; but a gate closed by a
// non-finite latent leaves non-finite activations behind, and 0 x nan products in the operands: the last writer of an element stores an
// exact zero instead when the gate scalar it is given reads 0 (loss.hip does the same for d(pred)).
// Operand tiles go global -> registers -> LDS (the loads of step t + 1 are in flight under the MFMAs of step t); the LDS images and the
// fragment reads are gemm_tiles.h's (A: K-contiguous, ds_read_b128; W: N-contiguous, ds_read_b64_tr_b16).  Rows >= M are never read
// (the plan's pad rows of dK | dV are being zeroed on the side stream at about the same time): their vectors are zeros made in registers.
#include "gemm_tiles.h"

namespace {
constexpr int CD_BN = 128, CD_BK = 64, CD_THREADS = 256;
constexpr int CD_TARGET_WG = 256;      // one workgroup per CU of the MI355X (a constant, not a device query: the split depends on shapes only)
constexpr int CD_MIN_STEPS = 4;        // K-steps of 64 per piece, at least

struct CdArgs {
  const bf16* A[2];
  const bf16* W[2];
  long lda[2], ldb[2];
  int steps[2];       // K_g / 64
  int nchunk[2];      // pieces of group g
  int chunk_steps;    // K-steps per piece (the last piece of a group may be shorter)
  float* out;         // slab [pieces][M][N] (or C itself when there is one piece)
  long ld_out;
  long piece_stride;  // floats between pieces in `out`
  int M, N;
  const float* gate;  // device scalar or null: 0 = the step's gradient gate is closed, the result is exact zeros (one-piece launches)
};

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

template <int RT>
__global__ __launch_bounds__(CD_THREADS) void cond_dgrad_kernel(const CdArgs p) {
  constexpr int BM = 64 * RT;
  constexpr int NA = 2 * RT;     // 16-byte vectors of the A tile per thread (BM * 8 / 256)
  constexpr int NB = 4;          // ... of the W tile (64 * 16 / 256)
  __shared__ __attribute__((aligned(16))) char smem[BM * CD_BK * 2 + CD_BK * CD_BN * 2];
  char* At = smem;
  char* Bt = smem + BM * CD_BK * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, g4 = lane >> 4;
  const int n0 = blockIdx.x * CD_BN, m0 = blockIdx.y * BM;
  int piece = blockIdx.z, grp = 0;
  if (piece >= p.nchunk[0]) { grp = 1; piece -= p.nchunk[0]; }
  const int s_begin = piece * p.chunk_steps;
  const int s_end = min(s_begin + p.chunk_steps, p.steps[grp]);
  const bf16* __restrict__ A = p.A[grp];
  const bf16* __restrict__ W = p.W[grp];
  const long lda = p.lda[grp], ldb = p.ldb[grp];

  // this thread's vectors: A rows ar + 32 i (k-vector akv), W k-rows bk + 16 i (column vector bv)
  const int ar = tid >> 3, akv = tid & 7;
  const int bk = tid >> 4, bv = tid & 15;
  const bool b_ok = n0 + bv * 8 < p.N;
  const bf16* a_ptr = A + (long)(m0 + ar) * lda + akv * 8;
  const bf16* b_ptr = W + (long)bk * ldb + n0 + bv * 8;
  u32x4 ra[NA], rb[NB];
  auto load_regs = [&](int step) {
    const long k0 = (long)step * CD_BK;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (m0 + ar + 32 * i < p.M) v = *(const u32x4*)(a_ptr + (long)(32 * i) * lda + k0);
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (b_ok) v = *(const u32x4*)(b_ptr + (k0 + 16 * i) * ldb);
      rb[i] = v;
    }
  };
  auto store_lds = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int r = ar + 32 * i;
      *(u32x4*)(At + r * (CD_BK * 2) + ((akv ^ kc_swz<CD_BK>(r)) << 4)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int k = bk + 16 * i;
      *(u32x4*)(Bt + k * (CD_BN * 2) + (nc_phys<CD_BN>(k, bv) << 4)) = rb[i];
    }
  };

  f32x4 acc[RT][8];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (s_begin < s_end) load_regs(s_begin);
  for (int s = s_begin; s < s_end; ++s) {
    store_lds();
    __syncthreads();
    if (s + 1 < s_end) load_regs(s + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[RT], fb[8];
#pragma unroll
      for (int i = 0; i < RT; ++i) fa[i] = frag_kc<CD_BK>(At, wave * (RT * 16) + i * 16 + l16, ks * 4 + g4);
#pragma unroll
      for (int j = 0; j < 8; ++j) fb[j] = frag_nc<CD_BN>(Bt, ks * 32 + g4 * 8, j * 16, l16);
#pragma unroll
      for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // partial tile -> this piece's slab slice: lane (g4, l16) holds rows 4 g4 + r, column l16 of every 16 x 16 fragment
  float* out = p.out + (long)blockIdx.z * p.piece_stride;
  const bool closed = p.gate && *p.gate == 0.f;
#pragma unroll
  for (int i = 0; i < RT; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + wave * (RT * 16) + i * 16 + g4 * 4 + r;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = n0 + j * 16 + l16;
        if (n < p.N) out[(long)m * p.ld_out + n] = closed ? 0.f : acc[i][j][r];
      }
    }
  }
}

// C[m][n] = slab[0][m][n] + slab[1][m][n] + ... in ascending piece order; four columns per thread (N % 8 == 0)
__global__ __launch_bounds__(256) void cond_dgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ C, long ldc, int M, int N,
                                                                int pieces, const float* __restrict__ gate) {
  const long nq = (long)N / 4, total = (long)M * nq;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long m = i / nq, q = i - m * nq;
  const long stride = (long)M * N;
  const float* s = slab + m * N + q * 4;
  f32x4 a = *(const f32x4*)s;
  for (int z = 1; z < pieces; ++z) a += *(const f32x4*)(s + z * stride);
  if (gate && *gate == 0.f) a = f32x4{0.f, 0.f, 0.f, 0.f};      // closed gradient gate: exact zeros, whatever the operands hold
  *(f32x4*)(C + m * ldc + q * 4) = a;
}

struct CdSplit { int rt, tiles_m, tiles_n, chunk_steps, nchunk[2], pieces; };
static CdSplit cd_split(int n, const int* K, int M, int N) {
  CdSplit s;
  s.rt = M > 256 ? 5 : (M + 63) / 64;
  if (s.rt < 1) s.rt = 1;
  s.tiles_m = (M + 64 * s.rt - 1) / (64 * s.rt);
  s.tiles_n = (N + CD_BN - 1) / CD_BN;
  long steps = 0;
  for (int g = 0; g < n; ++g) steps += K[g] / CD_BK;
  long want = CD_TARGET_WG / ((long)s.tiles_m * s.tiles_n);
  if (want < 1) want = 1;
  long cs = (steps + want - 1) / want;
  if (cs < CD_MIN_STEPS) cs = CD_MIN_STEPS;
  s.chunk_steps = (int)cs;
  s.nchunk[0] = s.nchunk[1] = 0;
  for (int g = 0; g < n; ++g) s.nchunk[g] = (int)((K[g] / CD_BK + cs - 1) / cs);
  s.pieces = s.nchunk[0] + s.nchunk[1];
  return s;
}
}  // namespace

size_t cond_dgrad_slab_floats(int n, const int* K, int M, int N) {
  if (n < 1 || n > 2 || M < 1 || N < 1) return 0;
  const CdSplit s = cd_split(n, K, M, N);
  return s.pieces > 1 ? (size_t)s.pieces * M * N : 0;
}

int launch_cond_dgrad(const CondDgradP& q, hipStream_t st) {
  ARG_CHECK(q.n >= 1 && q.n <= 2, "cond_dgrad: %d groups (1 or 2)", q.n);
  ARG_CHECK(q.M >= 1 && q.N >= 8 && q.N % 8 == 0, "cond_dgrad: M = %d, N = %d (M >= 1, N a multiple of 8)", q.M, q.N);
  ARG_CHECK(q.C && q.ldc >= q.N && q.ldc % 4 == 0 && ((uintptr_t)q.C & 15) == 0, "cond_dgrad: C must be 16-byte aligned with ldc >= N, a multiple of 4");
  for (int g = 0; g < q.n; ++g) {
    ARG_CHECK(q.K[g] >= CD_BK && q.K[g] % CD_BK == 0, "cond_dgrad: K[%d] = %d must be a positive multiple of 64", g, q.K[g]);
    ARG_CHECK(q.A[g] && q.W[g], "cond_dgrad: null operand of group %d", g);
    ARG_CHECK(q.lda[g] >= q.K[g] && q.lda[g] % 8 == 0 && q.ldb[g] >= q.N && q.ldb[g] % 8 == 0,
              "cond_dgrad: lda[%d] = %ld (>= K, multiple of 8), ldb = %ld (>= N, multiple of 8)", g, q.lda[g], q.ldb[g]);
    ARG_CHECK((((uintptr_t)q.A[g] | (uintptr_t)q.W[g]) & 15) == 0, "cond_dgrad: operands of group %d must be 16-byte aligned", g);
  }
  const CdSplit s = cd_split(q.n, q.K, q.M, q.N);
  ARG_CHECK(s.pieces <= 1 || q.slab, "cond_dgrad: %d pieces need a slab", s.pieces);
  ARG_CHECK(s.tiles_m <= 65535 && s.pieces <= 65535, "cond_dgrad: grid too large");
  CdArgs a;
  memset(&a, 0, sizeof(a));
  for (int g = 0; g < q.n; ++g) {
    a.A[g] = q.A[g]; a.W[g] = q.W[g]; a.lda[g] = q.lda[g]; a.ldb[g] = q.ldb[g];
    a.steps[g] = q.K[g] / CD_BK; a.nchunk[g] = s.nchunk[g];
  }
  a.chunk_steps = s.chunk_steps;
  a.M = q.M; a.N = q.N;
  if (s.pieces > 1) { a.out = q.slab; a.ld_out = q.N; a.piece_stride = (long)q.M * q.N; a.gate = nullptr; }      // (the reduce applies it)
  else { a.out = q.C; a.ld_out = q.ldc; a.piece_stride = 0; a.gate = q.gate; }
  const dim3 grid(s.tiles_n, s.tiles_m, s.pieces), block(CD_THREADS);
  switch (s.rt) {
    case 1: hipLaunchKernelGGL(cond_dgrad_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(cond_dgrad_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(cond_dgrad_kernel<3>, grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL(cond_dgrad_kernel<4>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(cond_dgrad_kernel<5>, grid, block, 0, st, a); break;
  }
  HIP_CHECK_RET(hipGetLastError());
  if (s.pieces > 1) {
    const long total = (long)q.M * (q.N / 4);
    hipLaunchKernelGGL(cond_dgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q.slab, q.C, q.ldc, q.M, q.N, s.pieces, q.gate);
    HIP_CHECK_RET(hipGetLastError());
  }
  return 0;
}
