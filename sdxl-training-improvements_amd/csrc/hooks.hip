// Single-kernel entry points: the test hooks and the experiment ABI of include/sdxlstep_diag.h, and the sdxl_op_* part of include/sdxlstep.h.
// One launch (or one op's few) on caller buffers; problems come from the same builders the plan uses (kernels.h), scratch from hook_scratch.
#include "capi.h"

// The hooks' scratch (the engine's is plan workspace): one buffer of the process, at least `bytes` and 256-byte aligned, kept between calls and
// only ever grown (hipFree waits for the launches that use the old one) -- a repeated call of one shape allocates nothing.  One stream at a
// time (a later hook reuses the bytes of an earlier one: only stream order keeps them apart); a hook that needs two regions carves them from
// one request.
static int hook_scratch(size_t bytes, void** out) {
  static char* buf = nullptr;
  static size_t cap = 0;
  if (bytes > cap) {
    if (buf) { (void)hipFree(buf); buf = nullptr; cap = 0; }
    HIP_CHECK_RET(hipMalloc((void**)&buf, bytes));
    cap = bytes;
  }
  *out = buf;
  return 0;
}
static int hook_floats(size_t n, float** out) { return hook_scratch(n * sizeof(float), (void**)out); }      // (split-K slabs, partial sums)
// the dense problem of sdxl_op_gemm / sdxl_op_gemm_sk / sdxl_debug_gemm_route from the plan's builders: every leading dimension is the row
// length; `bias` is the fp32 bias gradient of a TN problem
static int dense_problem(int form, const void* A, const void* B, void* C, int M, int N, int K, const void* bias, const void* resid, int accumulate,
                         GemmP* g) {
  const bf16 *a = (const bf16*)A, *b = (const bf16*)B, *r = (const bf16*)resid;
  ARG_CHECK(form == GEMM_NT || form == GEMM_NN || form == GEMM_TN, "gemm: unknown form %d", form);
  if (form == GEMM_NT) *g = linear_fwd_problem(a, K, b, C, N, M, N, K, (const bf16*)bias, r, N);
  else if (form == GEMM_NN) { *g = linear_dgrad_problem(a, K, b, C, N, M, N, K, r, N); g->bias = (const bf16*)bias; }
  else { *g = linear_wgrad_problem(a, M, b, N, (float*)C, M, N, K, (float*)bias); if (r) { g->resid = r; g->ldr = N; } }
  g->accumulate = accumulate;
  return 0;
}

extern "C" {

// ---- LoRA on caller buffers: the descriptor of one target (the device table of SDXL_DTYPE_LORA holds many) ----
static int lora_one(int out, int in, int rank, float scale, LoraP& q) {
  CHK(lora_check_shape("the operand", out, in, rank));
  ARG_CHECK(isfinite(scale), "lora: scale is not finite");
  memset(&q, 0, sizeof(q));
  q.n = 1; q.rank = rank; q.scale = scale;
  q.one.out = out; q.one.in = in; q.one.kind = LORA_KIND_PLAIN; q.one.nrows = out;
  q.tiles_m = lora_tiles_m(out, in); q.tiles_b = lora_tiles_b(out, in); q.tiles_a = lora_tiles_a(out, in);
  return 0;
}
// ... and of one target held in a packed layout: always the kind-aware kernels, also for LORA_KIND_PLAIN
static int lora_one_layout(int out, int in, int rank, float scale, int kind, int cg, int nrows, LoraP& q) {
  CHK(lora_one(out, in, rank, scale, q));
  ARG_CHECK(kind == LORA_KIND_PLAIN || kind == LORA_KIND_CONV3 || kind == LORA_KIND_GEGLU, "lora: kind %d (0 plain rows, 1 3x3 convolution, 2 GEGLU)", kind);
  ARG_CHECK(nrows >= out && (nrows == out || kind == LORA_KIND_CONV3), "lora: %d native rows for out = %d (only a convolution has padded rows)", nrows, out);
  if (kind == LORA_KIND_CONV3) ARG_CHECK(cg >= 1 && in == 9 * (long)cg, "lora: a 3x3 convolution with cin = %d has in = 9 cin, not %d", cg, in);
  if (kind == LORA_KIND_GEGLU) ARG_CHECK(cg >= 1 && out % 2 == 0 && (out / 2) % cg == 0, "lora: GEGLU rows [%d] are not whole groups of %d", out, cg);
  q.one.kind = kind; q.one.cg = kind == LORA_KIND_PLAIN ? 0 : cg; q.one.nrows = nrows; q.mapped = 1;
  q.tiles_m = lora_tiles_m(nrows, in);
  return 0;
}
// one body each for merge and project: `layout` = {kind, cg, native rows} of the _layout entry points (the kind-aware kernels, also for kind 0),
// NULL for the plain ones (q.mapped == 0: the MAPPED = false kernels)
static int lora_merge_hook(const void* base, const void* A, const void* B, void* w, int out, int in, int rank, float scale, const int* layout, void* st) {
  ARG_CHECK(aligned16(base) && aligned16(A) && aligned16(B) && aligned16(w), "lora_merge: every pointer must be 16-byte aligned and non-NULL");
  LoraP q;
  CHK(layout ? lora_one_layout(out, in, rank, scale, layout[0], layout[1], layout[2], q) : lora_one(out, in, rank, scale, q));
  q.w = (bf16*)w; q.base = (const bf16*)base; q.a = (const bf16*)A; q.b = (const bf16*)B;
  return launch_lora_merge(q, (hipStream_t)st);
}
static int lora_project_hook(const float* dw, const void* A, const void* B, float* dA, float* dB, int out, int in, int rank, float scale, const int* layout,
                             void* st) {
  ARG_CHECK(aligned16(dw) && aligned16(A) && aligned16(B) && aligned16(dA) && aligned16(dB),
            "lora_project: every pointer must be 16-byte aligned and non-NULL");
  LoraP q;
  CHK(layout ? lora_one_layout(out, in, rank, scale, layout[0], layout[1], layout[2], q) : lora_one(out, in, rank, scale, q));
  q.dw = dw; q.a = (const bf16*)A; q.b = (const bf16*)B; q.ga = dA; q.gb = dB;
  return launch_lora_project(q, (hipStream_t)st);
}
int sdxl_op_lora_merge_layout(const void* base, const void* A, const void* B, void* w, int out, int in, int rank, float scale, int kind, int cg,
                              int native_rows, void* st) {
  const int layout[3] = {kind, cg, native_rows};
  return lora_merge_hook(base, A, B, w, out, in, rank, scale, layout, st);
}
int sdxl_op_lora_project_layout(const float* dw, const void* A, const void* B, float* dA, float* dB, int out, int in, int rank, float scale, int kind,
                                int cg, int native_rows, void* st) {
  const int layout[3] = {kind, cg, native_rows};
  return lora_project_hook(dw, A, B, dA, dB, out, in, rank, scale, layout, st);
}
int sdxl_op_lora_merge(const void* base, const void* A, const void* B, void* w, int out, int in, int rank, float scale, void* st) {
  return lora_merge_hook(base, A, B, w, out, in, rank, scale, nullptr, st);
}
int sdxl_op_lora_project(const float* dw, const void* A, const void* B, float* dA, float* dB, int out, int in, int rank, float scale, void* st) {
  return lora_project_hook(dw, A, B, dA, dB, out, in, rank, scale, nullptr, st);
}

// ---- LoHa on caller buffers (csrc/loha.hip): the descriptor of one target, every offset 0 ----
static int loha_one(int out, int in, int rank, float scale, int kind, int group, LohaP& q) {
  CHK(loha_check_rank(rank));
  LoraP l;
  CHK(lora_one_layout(out, in, rank, scale, kind, group, out, l));
  memset(&q, 0, sizeof(q));
  q.n = 1; q.rank = rank; q.scale = scale;
  q.one.t = l.one;
  q.tiles_m = loha_tiles_m(out, in); q.tiles_b = loha_tiles_b(out, in); q.tiles_a = loha_tiles_a(out, in);
  return 0;
}
int sdxl_op_loha_merge(const void* base, const void* A1, const void* B1, const void* A2, const void* B2, void* w, int out, int in, int rank,
                       float scale, int kind, int group, void* st) {
  ARG_CHECK(aligned16(base) && aligned16(A1) && aligned16(B1) && aligned16(A2) && aligned16(B2) && aligned16(w),
            "loha_merge: every pointer must be 16-byte aligned and non-NULL");
  LohaP q;
  CHK(loha_one(out, in, rank, scale, kind, group, q));
  q.w = (bf16*)w; q.base = (const bf16*)base;
  q.a1 = (const bf16*)A1; q.b1 = (const bf16*)B1; q.a2 = (const bf16*)A2; q.b2 = (const bf16*)B2;
  return launch_loha_merge(q, (hipStream_t)st);
}
int sdxl_op_loha_project(const float* dw, const void* A1, const void* B1, const void* A2, const void* B2, float* dA1, float* dB1, float* dA2,
                         float* dB2, int out, int in, int rank, float scale, int kind, int group, void* st) {
  ARG_CHECK(aligned16(dw) && aligned16(A1) && aligned16(B1) && aligned16(A2) && aligned16(B2) && aligned16(dA1) && aligned16(dB1) &&
            aligned16(dA2) && aligned16(dB2), "loha_project: every pointer must be 16-byte aligned and non-NULL");
  LohaP q;
  CHK(loha_one(out, in, rank, scale, kind, group, q));
  q.dw = dw; q.a1 = (const bf16*)A1; q.b1 = (const bf16*)B1; q.a2 = (const bf16*)A2; q.b2 = (const bf16*)B2;
  q.ga1 = dA1; q.gb1 = dB1; q.ga2 = dA2; q.gb2 = dB2;
  return launch_loha_project(q, (hipStream_t)st);
}

int sdxl_op_lora_grad(const void* x, long ldx, const void* dy, long ldy, const void* A, const void* B, float* dA, float* dB, int M, int out, int in,
                      int rank, float scale, int accumulate, void* st) {
  ARG_CHECK(x && dy && aligned16(A) && aligned16(B) && aligned16(dA) && aligned16(dB), "lora_grad: A, B, dA, dB must be 16-byte aligned, x and dy non-NULL");
  CHK(lora_check_shape("the operand", out, in, rank));
  ARG_CHECK(isfinite(scale), "lora: scale is not finite");
  ARG_CHECK(M >= 1 && ldx >= in && ldy >= out, "lora_grad: M = %d, ldx = %ld (in = %d), ldy = %ld (out = %d)", M, ldx, in, ldy, out);
  LoraGradP q;
  memset(&q, 0, sizeof(q));
  q.n = 1; q.rank = rank; q.scale = scale; q.accumulate = accumulate != 0;
  q.one.out = out; q.one.in = in;
  q.x = (const bf16*)x; q.ldx = ldx; q.dy = (const bf16*)dy; q.ldy = ldy;
  q.M = M; q.Mp = lora_grad_mp(M); q.nchunk = lora_grad_chunks(M);
  q.tiles = lora_grad_tiles(out, in); q.reds = lora_grad_reds(out, in, rank);
  q.xvec = ((uintptr_t)x % 16 == 0 && ldx % 8 == 0) ? 1 : 0;
  q.yvec = ((uintptr_t)dy % 16 == 0 && ldy % 8 == 0) ? 1 : 0;
  q.a = (const bf16*)A; q.b = (const bf16*)B; q.ga = dA; q.gb = dB;
  // scratch of the hook (the engine's is plan workspace): one buffer of the process, kept between calls and only ever grown (hipFree
  // waits for the launches that use the old one), so that repeated calls of one shape enqueue three launches and nothing else
  const size_t tu_bytes = (lora_grad_tu_elems(1, rank, M) * sizeof(bf16) + 255) / 256 * 256;
  char* scratch;
  CHK(hook_scratch(tu_bytes + lora_grad_part_floats(out, in, rank, M) * sizeof(float), (void**)&scratch));
  q.tu = (bf16*)scratch; q.part = (float*)(scratch + tu_bytes);
  return launch_lora_grad(q, (hipStream_t)st);
}

int sdxl_op_gemm(int form, const void* A, const void* B, void* C, int M, int N, int K, const void* bias,
                 const void* resid, int accumulate, int splitk, void* st) {
  GemmP g;
  CHK(dense_problem(form, A, B, C, M, N, K, bias, resid, accumulate, &g));
  if (form == GEMM_TN) g.splitk = splitk <= 0 ? linear_wgrad_splitk(M, N, K) : splitk;     // (<= 0: the plan's choice)
  else if (splitk > 1) g.splitk = splitk;
  if (g.splitk > 1) CHK(hook_floats(gemm_slab_floats(M, N, 1, g.splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}

int sdxl_op_cond_dgrad(int n, const void* const* A, const long* lda, const void* const* W, const long* ldb, const int* K, float* C, long ldc,
                       int M, int N, void* st) {
  ARG_CHECK(n >= 1 && n <= 2 && A && lda && W && ldb && K, "cond_dgrad: 1 or 2 groups, no null array");
  CondDgradP q;
  memset(&q, 0, sizeof(q));
  q.n = n;
  for (int g = 0; g < n; ++g) { q.A[g] = (const bf16*)A[g]; q.lda[g] = lda[g]; q.W[g] = (const bf16*)W[g]; q.ldb[g] = ldb[g]; q.K[g] = K[g]; }
  q.C = C; q.ldc = ldc; q.M = M; q.N = N;
  ARG_CHECK(M >= 1 && N >= 8, "cond_dgrad: M = %d, N = %d", M, N);
  for (int g = 0; g < n; ++g) ARG_CHECK(K[g] >= 64 && K[g] % 64 == 0, "cond_dgrad: K[%d] = %d must be a positive multiple of 64", g, K[g]);
  const size_t need = cond_dgrad_slab_floats(n, K, M, N);
  if (need) CHK(hook_floats(need, &q.slab));
  return launch_cond_dgrad(q, (hipStream_t)st);
}

// ---- additional skip residuals (residual.hip) on caller buffers: the two launches of ConcatOp with a residual request ----
int sdxl_op_concat_residual(const void* a, int Ca, const void* b, int Cb, const void* ra, const void* rb, int rdtype, void* o, int B, int HW, void* st) {
  return launch_concat_residual((const bf16*)a, Ca, (const bf16*)b, Cb, ra, rb, rdtype, (bf16*)o, B, HW, (hipStream_t)st);
}
int sdxl_op_concat_residual_grad(const void* g, int Ca, int Cb, float* dra, float* drb, const float* gate_dev, int B, int HW, void* st) {
  return launch_residual_grad((const bf16*)g, Ca, Cb, dra, drb, gate_dev, B, HW, (hipStream_t)st);
}

// ---- input gradient (input_dgrad.hip) on caller buffers: the launch of conv_in's backward with a sdxl_batch_din request ----
int sdxl_op_input_dgrad(const void* dy, const void* w, float* dx, const float* gate_dev, int B, int H, int W, int in_channels, int Cout, void* st) {
  return launch_input_dgrad((const bf16*)dy, (const bf16*)w, dx, gate_dev, B, H, W, in_channels, Cout, (hipStream_t)st);
}
int sdxl_debug_input_dgrad_operands(sdxl_handle* h, size_t* dy_ws_byte_off, size_t* w_elem_off, int* Cout) {
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(dy_ws_byte_off && w_elem_off && Cout, "null output");
  const Plan::CondSrc& s = h->e.cur->din_src;
  ARG_CHECK(s.dy_off != NONE, "input dgrad operands: the plan has no backward for conv_in");
  *dy_ws_byte_off = s.dy_off; *w_elem_off = s.w.off; *Cout = s.K;
  return 0;
}

int sdxl_debug_cond_operands(sdxl_handle* h, int which, int g, int* n_groups, size_t* a_ws_byte_off, long* lda, size_t* w_elem_off, long* ldb,
                             int* K) {
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(n_groups && a_ws_byte_off && lda && w_elem_off && ldb && K, "null output");
  const Plan& p = *h->e.cur;
  const int n = which == 0 ? p.cond_nkv : 1;
  ARG_CHECK((which == 0 || which == 1) && g >= 0 && g < n, "cond operands: which = %d, group %d of %d", which, g, n);
  const Plan::CondSrc& cs = which == 0 ? p.cond_kv[g] : p.cond_add;
  *n_groups = n; *a_ws_byte_off = cs.dy_off; *lda = cs.lda; *w_elem_off = cs.w.off; *ldb = cs.ldb; *K = cs.K;
  return 0;
}

// ---- the plan map: every op of the current plan described from its own fields (Op::describe); nothing is launched or reserved ----
int sdxl_debug_plan_num_ops(sdxl_handle* h, int* n) {
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(n, "null output");
  *n = (int)h->e.cur->ops.size();
  return 0;
}
int sdxl_debug_plan_op(sdxl_handle* h, int i, sdxl_plan_op_desc* out, size_t out_bytes) {
  ARG_CHECK(out_bytes == sizeof(sdxl_plan_op_desc), "plan op: the caller's descriptor has %zu bytes, the library's %zu", out_bytes, sizeof(sdxl_plan_op_desc));
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(out, "null output");
  const Plan& p = *h->e.cur;
  ARG_CHECK(i >= 0 && i < (int)p.ops.size(), "plan op %d out of range (the plan has %d)", i, (int)p.ops.size());
  memset(out, 0, sizeof(*out));
  size_t* const offs[] = {&out->dy_off, &out->dx_out, &out->dx_addend, &out->dres_out, &out->dres_addend, &out->d3_out, &out->d3_addend, &out->dy32_off,
                          &out->w_off, &out->b_off, &out->stats_off, &out->lse_off, &out->delta_off, &out->rv32_off, &out->planar_off, &out->weff_off,
                          &out->dweff_off, &out->s2_planar_off};
  for (size_t* o : offs) *o = SDXL_PLAN_NONE;
  for (int r = 0; r < SDXL_PLAN_ROLES; ++r) plan_describe_tensor(out->t[r], nullptr);
  out->intact_after_step = ~0u;
  const Op& op = *p.ops[i];
  out->seg = op.seg; out->hoist_fwd = op.hoist_fwd ? 1 : 0;
  op.describe(p, out);
  return 0;
}
int sdxl_debug_plan_tail(sdxl_handle* h, sdxl_plan_tail* out, size_t out_bytes) {
  ARG_CHECK(out_bytes == sizeof(sdxl_plan_tail), "plan tail: the caller's struct has %zu bytes, the library's %zu", out_bytes, sizeof(sdxl_plan_tail));
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(out, "null output");
  const Plan& p = *h->e.cur;
  memset(out, 0, sizeof(*out));
  out->B = p.B; out->H = p.H; out->W = p.W; out->ctx = p.ctx;
  plan_describe_tensor(out->x_in, p.x_in); plan_describe_tensor(out->pred, p.pred); plan_describe_tensor(out->ehs, p.ehs);
  out->tp32_off = p.tp32_off; out->tp32_bytes = p.tp32_bytes; out->t_off = p.t_off; out->tid_off = p.tid_off; out->loss_off = p.loss_off;
  out->workspace_bytes = p.ws_bytes;
  return 0;
}
int sdxl_debug_plan_loss(sdxl_handle* h, sdxl_plan_loss* out, size_t out_bytes) {
  ARG_CHECK(out_bytes == sizeof(sdxl_plan_loss), "plan loss: the caller's struct has %zu bytes, the library's %zu", out_bytes, sizeof(sdxl_plan_loss));
  H_CHECK(h);
  ARG_CHECK(h->e.cur, "no plan: call sdxl_plan first");
  ARG_CHECK(out, "null output");
  const Plan& p = *h->e.cur;
  memset(out, 0, sizeof(*out));
  out->loss_part_off = p.loss_part_off; out->ps_loss_off = p.ps_loss_off; out->mask_norm_off = p.mask_norm_off;
  out->in_lat_off = p.in_lat_off; out->in_noise_off = p.in_noise_off; out->in_nin_off = p.in_nin_off; out->in_sig_off = p.in_sig_off;
  out->in_tag_off = p.in_tag_off; out->in_sw_off = p.in_sw_off; out->in_hc_off = p.in_hc_off; out->in_mask_off = p.in_mask_off;
  out->in_cond_off = p.in_cond_off;
  out->part_floats = loss_part_floats(p.B, p.H * p.W); out->ps_slots = loss_ps_slots(p.B, p.H * p.W);
  // the loss kernels of the last forward read what StepState::b holds: the staged latents of this plan, or the caller's pointer
  out->staged = !h->step.valid ? -1 : (p.in_lat_off != NONE && h->step.b.latents == p.F(p.in_lat_off)) ? 1 : 0;
  return 0;
}

int sdxl_op_wgrad_group(int n, const void* const* dy, const void* const* x, float* const* dw, float* const* dbias, int Mo, int No,
                        int rows, int accumulate, void* st) {
  ARG_CHECK(n >= 1 && n <= GEMM_MAX_GROUP, "wgrad group of %d (1..%d)", n, GEMM_MAX_GROUP);
  GemmP v[GEMM_MAX_GROUP];
  for (int i = 0; i < n; ++i) v[i] = linear_wgrad_problem((const bf16*)dy[i], Mo, (const bf16*)x[i], No, dw[i], Mo, No, rows, dbias ? dbias[i] : nullptr);
  GemmP g = v[0];
  g.accumulate = accumulate;
  gemm_fill_group(g, v, n);
  return launch_gemm(g, (hipStream_t)st);
}

int sdxl_op_conv3x3_fwd(const void* x, const void* w, const void* bias, void* y, int B, int H, int W, int Cin, int Cout,
                        int stride, void* st) {
  GemmP g = conv3x3_fwd_problem(B, H, W, Cin, Cout, stride);
  g.A = (const bf16*)x; g.B = (const bf16*)w; g.C = y;
  g.bias = (const bf16*)bias;
  g.splitk = conv3x3_fwd_splitk(B, H, W, Cin, Cout, stride);
  if (g.splitk > 1) CHK(hook_floats(gemm_slab_floats(g.M, Cout, 1, g.splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}
// y = conv3x3(upsample2x(x)) and its input gradient without the upsampled image (GemmP::up2); weff [Cout][16][Cin] and planar
// [4 B H W][Cout] bf16 are scratch of the caller (weff written by the forward, read by the dgrad)
int sdxl_op_upconv3x3_fwd(const void* x, const void* w, const void* bias, void* weff, void* planar, void* y, int B, int H, int W,
                          int Cin, int Cout, void* st) {
  const int Mp = 4 * (int)upconv_plane_rows(B, H, W);
  int splitk = upconv3x3_fwd_splitk(B, H, W, Cin, Cout);
  float* slab = nullptr;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(Mp, Cout, 1, splitk), &slab));
  return launch_upconv3x3_fwd((const bf16*)x, (const bf16*)w, (const bf16*)bias, (bf16*)weff, (bf16*)planar, (bf16*)y, B, H, W, Cin, Cout,
                              splitk, slab, (hipStream_t)st);
}
int sdxl_op_upconv3x3_dgrad(const void* dy, const void* weff, void* planar, void* dx, const void* addend, int B, int H, int W, int Cin,
                            int Cout, void* st) {
  int splitk = upconv3x3_dgrad_splitk(B, H, W, Cin, Cout);
  float* slab = nullptr;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(B * H * W, Cin, 1, splitk), &slab));
  return launch_upconv3x3_dgrad((const bf16*)dy, (const bf16*)weff, (bf16*)planar, (bf16*)dx, (const bf16*)addend, B, H, W, Cin, Cout, splitk,
                                slab, 0, (hipStream_t)st);
}
#ifdef SDXL_DIAG
// stride-2 3x3 convolution through the fast gather on the four phase planes of x (GemmP::up2 == 3); xplanar [4 * roundup(B*(H/2)*(W/2), 128)][Cin]
// bf16: written by _fwd, read by _wgrad
int sdxl_op_conv3x3_s2_fwd(const void* x, const void* w, const void* bias, void* xplanar, void* y, int B, int H, int W, int Cin, int Cout,
                           void* st) {
  return launch_conv3x3_s2_fwd((const bf16*)x, (const bf16*)w, (const bf16*)bias, (bf16*)xplanar, (bf16*)y, B, H, W, Cin, Cout, (hipStream_t)st);
}
int sdxl_op_conv3x3_s2_wgrad(const void* dy, const void* xplanar, float* dw, float* dbias, int accumulate, int B, int H, int W, int Cin,
                             int Cout, int splitk, void* st) {
  float* slab = nullptr;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(Cout, Cin, 9, splitk), &slab));
  return launch_conv3x3_s2_wgrad((const bf16*)dy, (const bf16*)xplanar, dw, dbias, nullptr, 1.f, accumulate, B, H, W, Cin, Cout, splitk, slab,
                                 (hipStream_t)st);
}
#endif
// input gradient of the stride-2 3x3 convolution by output phase (GemmP::up2 == 2); planar [4 * roundup(B*(H/2)*(W/2), 128)][Cin] scratch
int sdxl_op_conv3x3_s2_dgrad(const void* dy, const void* w, void* planar, void* dx, const void* addend, int B, int H, int W, int Cin,
                             int Cout, void* st) {
  return launch_conv3x3_s2_dgrad((const bf16*)dy, (const bf16*)w, (bf16*)planar, (bf16*)dx, (const bf16*)addend, B, H, W, Cin, Cout, 0,
                                 (hipStream_t)st);
}
// the weight / bias gradient of the same pair from `planar` as sdxl_op_upconv3x3_dgrad left it (the de-interleaved dy) and the
// low-resolution x; dweff [Cout][16][Cin] fp32 scratch; dw [Cout][9][Cin] (= or +=), dbias += (may be NULL)
int sdxl_op_upconv3x3_wgrad(const void* planar, const void* x, float* dweff, float* dw, float* dbias, int accumulate, int B, int H, int W,
                            int Cin, int Cout, int splitk, void* st) {
  float* slab = nullptr;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(Cout, Cin, 16, splitk), &slab));
  return launch_upconv3x3_wgrad((const bf16*)planar, (const bf16*)x, dweff, dw, dbias, nullptr, 1.f, accumulate, B, H, W, Cin, Cout, splitk,
                                slab, (hipStream_t)st);
}
int sdxl_op_conv3x3_dgrad(const void* dy, const void* w, void* dx, int B, int H, int W, int Cin, int Cout, int stride,
                          void* st) {
  GemmP g = conv3x3_dgrad_problem(B, H, W, Cin, Cout, stride);
  g.A = (const bf16*)dy; g.B = (const bf16*)w; g.C = dx;
  g.splitk = conv3x3_dgrad_splitk(B, H, W, Cin, Cout, stride);
  if (g.splitk > 1) CHK(hook_floats(gemm_slab_floats(g.M, Cin, 1, g.splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}
int sdxl_op_conv3x3_wgrad(const void* x, const void* dy, float* dw, int B, int H, int W, int Cin, int Cout, int stride,
                          int splitk, void* st) {
  GemmP g = conv3x3_wgrad_problem(B, H, W, Cin, Cout, stride);
  g.A = (const bf16*)dy; g.B = (const bf16*)x; g.C = dw;
  g.splitk = splitk; g.accumulate = 1;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(Cout, Cin, 9, splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}

int sdxl_op_conv3x3_wgrad2(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout, int stride,
                           int splitk, int accumulate, void* st) {
  GemmP g = conv3x3_wgrad_problem(B, H, W, Cin, Cout, stride);
  g.A = (const bf16*)dy; g.B = (const bf16*)x; g.C = dw;
  g.accumulate = accumulate; g.bias_grad = dbias;
  if (splitk <= 0) splitk = conv3x3_wgrad_splitk(B, H, W, Cin, Cout, stride);      // the plan's choice
  g.splitk = splitk;
  if (splitk > 1) CHK(hook_floats(gemm_slab_floats(Cout, Cin, 9, splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}

int sdxl_op_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int heads, int Nq,
                          int Nk, long ldq, long ldk, long ldv, long ldo, void* st) {
  AttnP a;
  memset(&a, 0, sizeof(a));
  a.Q = (const bf16*)q; a.K = (const bf16*)k; a.V = (const bf16*)v; a.O = (bf16*)o; a.LSE = lse;
  a.B = B; a.H = heads; a.Nq = Nq; a.Nk = Nk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  return launch_attn_fwd(a, (hipStream_t)st);
}
int sdxl_op_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                          float* delta, void* dq, void* dk, void* dv, int B, int heads, int Nq, int Nk, long ldq,
                          long ldk, long ldv, long ldo, void* st) {
  AttnP a;
  memset(&a, 0, sizeof(a));
  a.Q = (const bf16*)q; a.K = (const bf16*)k; a.V = (const bf16*)v; a.O = (bf16*)o; a.LSE = (float*)lse;
  a.B = B; a.H = heads; a.Nq = Nq; a.Nk = Nk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.dO = (const bf16*)d_o; a.lddo = ldo; a.Delta = delta;
  a.dQ = (bf16*)dq; a.dK = (bf16*)dk; a.dV = (bf16*)dv; a.lddq = ldq; a.lddk = ldk; a.lddv = ldv;
  a.qsplit = attn_pick_qsplit(B, heads, Nq, Nk);
  if (a.qsplit > 1) CHK(hook_floats(attn_part_floats(B, heads, Nk, a.qsplit), &a.part));
  return launch_attn_bwd(a, (hipStream_t)st);
}

int sdxl_op_groupnorm_fwd(const void* x, void* y, const void* gamma, const void* beta, float* stats, float* ws, int B,
                          int HW, int C, int G, float eps, int silu, void* st) {
  return launch_groupnorm_fwd((const bf16*)x, (bf16*)y, (const bf16*)gamma, (const bf16*)beta, stats, ws, B, HW, C, G, eps,
                              silu, (hipStream_t)st);
}
int sdxl_op_groupnorm_bwd(const void* x, const void* dy, const void* gamma, const void* beta, const float* stats, void* dx,
                          float* dgamma, float* dbeta, float* ws, int B, int HW, int C, int G, int silu, int accumulate,
                          void* st) {
  return launch_groupnorm_bwd((const bf16*)x, (const bf16*)dy, (const bf16*)gamma, (const bf16*)beta, stats, (bf16*)dx,
                              accumulate ? (const bf16*)dx : nullptr, dgamma, dbeta, ws, B, HW, C, G, silu, (hipStream_t)st);
}
int sdxl_op_layernorm_fwd(const void* x, void* y, const void* gamma, const void* beta, float* stats, int M, int C,
                          float eps, void* st) {
  return launch_layernorm_fwd((const bf16*)x, (bf16*)y, (const bf16*)gamma, (const bf16*)beta, stats, M, C, eps,
                              (hipStream_t)st);
}
int sdxl_op_layernorm_bwd(const void* x, const void* dy, const void* gamma, const float* stats, void* dx, float* dgamma,
                          float* dbeta, int M, int C, int accumulate, void* st) {
  if (!dgamma)
    return launch_layernorm_bwd((const bf16*)x, (const bf16*)dy, (const bf16*)gamma, stats, (bf16*)dx,
                                accumulate ? (const bf16*)dx : nullptr, nullptr, nullptr, M, C, (hipStream_t)st);
  ARG_CHECK(dbeta, "layernorm bwd: dgamma and dbeta go together");
  if (KNOB(10) == 1 || KNOB(10) == 3) {     // (A/B runs) lean dx kernel + parameter gradients as a pass of their own; the plan's default is the one-pass form below
    CHK(launch_layernorm_bwd((const bf16*)x, (const bf16*)dy, (const bf16*)gamma, stats, (bf16*)dx,
                             accumulate ? (const bf16*)dx : nullptr, nullptr, nullptr, M, C, (hipStream_t)st));
    if (KNOB(10) == 3) return launch_layernorm_param_grads((const bf16*)x, (const bf16*)dy, stats, dgamma, dbeta, M, C, (hipStream_t)st);
    LnRedBatch b;
    b.n = 1;
    float* part;
    CHK(hook_floats(layernorm_bwd_part_floats(M, C), &part));
    b.e[0].part = part; b.e[0].dgamma = dgamma; b.e[0].dbeta = dbeta; b.e[0].C = C; b.e[0].nblk = layernorm_param_partial_rows(M, C);
    CHK(launch_layernorm_param_partials((const bf16*)x, (const bf16*)dy, stats, part, M, C, (hipStream_t)st));
    return launch_ln_param_reduce(b, (hipStream_t)st);
  }
  LnRedBatch b;
  b.n = 1;
  float* part;
  CHK(hook_floats(layernorm_bwd_part_floats(M, C), &part));
  b.e[0].part = part; b.e[0].dgamma = dgamma; b.e[0].dbeta = dbeta; b.e[0].C = C;
  CHK(launch_layernorm_bwd((const bf16*)x, (const bf16*)dy, (const bf16*)gamma, stats, (bf16*)dx,
                           accumulate ? (const bf16*)dx : nullptr, part, &b.e[0].nblk, M, C, (hipStream_t)st));
  return launch_ln_param_reduce(b, (hipStream_t)st);
}
int sdxl_op_ff_geglu_fwd(const void* x, const void* w1, const void* b1, void* u, void* g, int M, int K, int C4, int group,
                         void* st) {
  GemmP p = linear_fwd_problem((const bf16*)x, K, (const bf16*)w1, u, 2L * C4, M, 2 * C4, K, (const bf16*)b1, nullptr, 0);
  gemm_attach_geglu_fwd(p, group, (bf16*)g, C4);
  return launch_gemm(p, (hipStream_t)st);
}
int sdxl_op_ff_geglu_bwd(const void* dy, const void* w2, const void* u, void* du, int M, int C, int C4, int group,
                         void* st) {
  GemmP p = linear_dgrad_problem((const bf16*)dy, C, (const bf16*)w2, du, C4, M, C4, C, nullptr, 0);
  gemm_attach_geglu_bwd(p, group, (bf16*)u, 2L * C4);
  return launch_gemm(p, (hipStream_t)st);
}

int sdxl_op_loss(const sdxl_loss_config* lc, const sdxl_batch* b, void* unet_in, const void* pred, void* dpred,
                 float grad_scale, float* out8, int phase, void* st) {
  ARG_CHECK(lc && b, "null argument");
  sdxl_loss_config full;
  CHK(read_loss_config(lc, &full));
  lc = &full;
  LossP L;
  memset(&L, 0, sizeof(L));
  L.method = lc->method; L.prediction_type = lc->prediction_type; L.use_min_snr = lc->use_min_snr;
  L.min_snr_gamma = lc->min_snr_gamma; L.use_ztsnr = lc->use_ztsnr;
  L.B = b->B; L.HW = b->H * b->W; L.C = 4;
  L.latents = b->latents; L.noise = b->noise; L.sigma = b->sigma_or_t; L.tag_w = b->tag_weights;
  L.unet_in = (bf16*)unet_in; L.pred = (const bf16*)pred; L.dpred = (bf16*)dpred;
  L.grad_scale = grad_scale; L.out = out8;
  CHK(check_loss_ext(lc, b));
  fill_loss_ext(lc, b, L);
  const float* icond = nullptr;
  int ncond = 0;
  if (phase == 0) {      // extra input channels: no handle here, so cond_channels is their number (unet_in is [B*HW][input_cs(4 + ncond)])
    read_input_cond(b, &icond, &ncond);
    ARG_CHECK(ncond >= 0 && ncond <= 12, "input_cond: cond_channels %d outside 0 .. 12", ncond);
    ARG_CHECK(ncond == 0 || icond, "input_cond is missing: cond_channels = %d", ncond);
    ARG_CHECK(ncond > 0 || !icond, "input_cond must be NULL with cond_channels = 0 (in_channels = 4)");
  }
  // the partial rows of phase 1, and behind them the [B] normaliser that masked_mean's phase 1 leaves for its phase 2
  if (phase == 1 || (phase == 2 && L.mask && L.mask_norm == 1)) {
    ARG_CHECK(L.B > 0 && L.HW > 0, "loss: empty batch");
    CHK(hook_floats(loss_part_floats(L.B, L.HW) + (size_t)L.B, &L.part));
    L.mnorm = L.part + loss_part_floats(L.B, L.HW);
  }
  if (phase == 0) return launch_loss_prepare(L, (hipStream_t)st, icond, ncond);
  if (phase == 1) return launch_loss_fwd(L, (hipStream_t)st);
  if (phase == 2) return launch_loss_bwd(L, (hipStream_t)st);
  ARG_CHECK(false, "phase %d", phase);
}

int sdxl_op_sampler_step(float* x, const void* pred, void* x_in, int B, int H, int W, const sdxl_sampler_step* s, void* st) {
  ARG_CHECK(s, "null argument");
  ARG_CHECK(B > 0 && H > 0 && W > 0, "sampler: empty batch");
  sdxl_sampler_step_ext t;      // the caller's struct as far as its flag says it goes, with x set
  memset(&t, 0, sizeof(t));
  memcpy(&t, s, (s->init & SDXL_SAMPLER_EXT) ? sizeof(sdxl_sampler_step_ext) : sizeof(sdxl_sampler_step));
  t.base.x = x;
  SamplerP q;
  CHK(fill_sampler(&t.base, s->cfg ? 2 * B : B, H * W, q));      // B = samples here: the images hold 2B rows of HW with cfg
  q.pred = (const bf16*)pred; q.x_in = (bf16*)x_in;
  if (!q.init && q.rescale != 0.f) CHK(hook_floats(sampler_part_floats(B, H * W), &q.part));
  return launch_sampler_step(q, (hipStream_t)st);
}
int sdxl_probe_layout(void* out, void* st) { return probe_layout(out, (hipStream_t)st); }
int sdxl_op_exchange_shadow(void* buf, size_t bytes, int workgroups, int lds_bytes, float busy_us, void* st) {
  return launch_exchange_shadow(buf, bytes, workgroups, lds_bytes, busy_us, (hipStream_t)st);
}
// test hook (include/sdxlstep_diag.h part 1): sdxl_op_gemm's NT / NN forms with explicit leading dimensions (padded activations, as the plan's
// feed-forward hidden tensors are) and a forced configuration for this launch only (0: the policy)
int sdxl_op_gemm_ld(int form, const void* A, const void* B, void* C, int M, int N, int K, long lda, long ldb, long ldc, const void* bias,
                    const void* resid, long ldr, int cfg, void* st) {
  ARG_CHECK(form == GEMM_NT || form == GEMM_NN, "gemm_ld: NT / NN only (form %d)", form);
  GemmP g;
  if (form == GEMM_NT) g = linear_fwd_problem((const bf16*)A, lda, (const bf16*)B, C, ldc, M, N, K, (const bf16*)bias, (const bf16*)resid, ldr);
  else { g = linear_dgrad_problem((const bf16*)A, lda, (const bf16*)B, C, ldc, M, N, K, (const bf16*)resid, ldr); g.bias = (const bf16*)bias; }
  g.ldb = ldb;      // (the hook's weight may have padded rows too)
  g.cfg = cfg;
  return launch_gemm(g, (hipStream_t)st);
}
// ---- the time-embedding path on caller buffers (include/sdxlstep_diag.h part 1) ----
// what a hook refuses of a row vector before any launch: the kernels load it in 16-byte pieces and divide the row by rows_per_batch
static int rowvec_check(const char* who, const void* rowvec, long ldv, int rows_per_batch, long M, int N) {
  ARG_CHECK(aligned16(rowvec), "%s: the row vector must be 16-byte aligned and non-NULL", who);
  ARG_CHECK(ldv % 8 == 0 && ldv >= N, "%s: ldv = %ld must be a multiple of 8 and at least N = %d", who, ldv, N);
  ARG_CHECK(rows_per_batch >= 1 && M % rows_per_batch == 0, "%s: %ld rows are not whole samples of %d rows", who, M, rows_per_batch);
  return 0;
}
// the NT problem of a resnet's first convolution as a dense launch: C = bf16(A . B^T + bias + rowvec[m / rows_per_batch] + resid), the vector a
// column slice of a wider [M / rows_per_batch][ldv] matrix; cfg as sdxl_op_gemm_ld's, splitk > 1 as sdxl_op_gemm's
int sdxl_op_gemm_rowvec(int form, const void* A, const void* B, void* C, int M, int N, int K, const void* bias, const void* resid, const void* rowvec,
                        long ldv, int rows_per_batch, int splitk, int cfg, void* st) {
  ARG_CHECK(form == GEMM_NT, "gemm_rowvec: NT only (form %d)", form);
  ARG_CHECK(M > 0 && N > 0 && K > 0, "gemm_rowvec: empty problem M=%d N=%d K=%d", M, N, K);
  CHK(rowvec_check("gemm_rowvec", rowvec, ldv, rows_per_batch, M, N));
  GemmP g = linear_fwd_problem((const bf16*)A, K, (const bf16*)B, C, N, M, N, K, (const bf16*)bias, (const bf16*)resid, N);
  g.rowvec = (const bf16*)rowvec; g.ldv = ldv; g.rows_per_batch = rows_per_batch;
  g.cfg = cfg;
  if (splitk > 1) {
    g.splitk = splitk;
    CHK(hook_floats(gemm_slab_floats(M, N, 1, splitk), &g.slab));
  }
  return launch_gemm(g, (hipStream_t)st);
}
// ... and as ConvOp::fwd builds it: stride 1, the plan's split factor, one vector per image
int sdxl_op_conv3x3_fwd_rowvec(const void* x, const void* w, const void* bias, const void* rowvec, long ldv, void* y, int B, int H, int W, int Cin,
                               int Cout, void* st) {
  ARG_CHECK(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv3x3_fwd_rowvec: empty problem");
  CHK(rowvec_check("conv3x3_fwd_rowvec", rowvec, ldv, H * W, (long)B * H * W, Cout));
  GemmP g = conv3x3_fwd_problem(B, H, W, Cin, Cout, 1);
  g.A = (const bf16*)x; g.B = (const bf16*)w; g.C = y;
  g.bias = (const bf16*)bias;
  g.rowvec = (const bf16*)rowvec; g.ldv = ldv; g.rows_per_batch = H * W;
  g.splitk = conv3x3_fwd_splitk(B, H, W, Cin, Cout, 1);
  if (g.splitk > 1) CHK(hook_floats(gemm_slab_floats(g.M, Cout, 1, g.splitk), &g.slab));
  return launch_gemm(g, (hipStream_t)st);
}
// the backward of that broadcast (and, as one batch with ld_out = 0, the up-sampler's bias gradient): out[b][n] += sum over the rows of batch b
int sdxl_op_colsum(const void* x, long ldx, float* out, long ld_out, int batches, int rows, int N, void* st) {
  ARG_CHECK(batches >= 1 && batches <= LN_RED_MAX, "colsum: %d batches (1 .. %d)", batches, LN_RED_MAX);
  ARG_CHECK(aligned16(x) && out && ((uintptr_t)out & 3) == 0, "colsum: x must be 16-byte aligned, out non-NULL");
  ARG_CHECK(rows >= 1 && N >= 8 && N % 8 == 0 && ldx >= N && ldx % 8 == 0, "colsum: rows = %d, N = %d, ldx = %ld", rows, N, ldx);
  ARG_CHECK(batches == 1 || ld_out >= N, "colsum: ld_out = %ld holds no row of %d sums", ld_out, N);
  float* part;
  CHK(hook_floats(colsum_part_floats(batches, rows, N), &part));
  return launch_colsum_f32_batched((const bf16*)x, out, batches, rows, N, ldx, ld_out, part, (hipStream_t)st);
}
// the sinusoidal embedding: out [rows][ldo] bf16, columns [0, dim) = cos | sin of t[r] exp(-ln(1e4) k / (dim / 2))
int sdxl_op_sincos(const float* t, void* out, int rows, int dim, long ldo, void* st) {
  ARG_CHECK(t && out && rows >= 1 && dim >= 2 && ldo >= dim && (long)rows * dim < (1L << 31), "sincos: rows = %d, dim = %d, ldo = %ld", rows, dim, ldo);
  return launch_sincos(t, (bf16*)out, rows, dim, ldo, (hipStream_t)st);
}
// test hook (include/sdxlstep_diag.h part 1): the NN dgrad with the Delta epilogue, as LinearOp::bwd launches it for a self-attention
// layer's out-projection
int sdxl_op_linear_dgrad_delta(const void* dy, const void* w, const void* o, const void* addend, void* d_o, float* delta, int B, int Nq,
                               int N, int K, void* st) {
  ARG_CHECK(dy && w && o && d_o && delta && B > 0 && Nq > 0 && N % 128 == 0 && K % 64 == 0, "linear_dgrad_delta: B=%d Nq=%d N=%d K=%d", B, Nq, N, K);
  GemmP g = linear_dgrad_problem((const bf16*)dy, K, (const bf16*)w, d_o, N, B * Nq, N, K, (const bf16*)addend, N);
  gemm_attach_delta(g, (const bf16*)o, N, delta, Nq, N / 64);
  return launch_gemm(g, (hipStream_t)st);
}
// test hook (include/sdxlstep_diag.h part 1): what launch_gemm would run for the problem a launch-log line describes.  The operands gemm_route never
// looks at are dense and stand on one aligned dummy word; no device is touched.
int sdxl_debug_gemm_route(const sdxl_gemm_desc* d, sdxl_gemm_route* out) {
  ARG_CHECK(d && out, "gemm_route: null argument");
  alignas(16) static float word[4];
  GemmP g;
  CHK(dense_problem(d->form, word, word, word, d->M, d->N, d->K, nullptr, nullptr, 0, &g));      // taps == 1: the linear builders' leading dimensions
  g.taps = d->taps; g.cfg = d->cfg;
  g.ldb *= d->taps;      // the weight's (NT / NN) or the gathered image's rows hold every tap, and so do the weight gradient's
  if (d->form == GEMM_TN) g.ldc *= d->taps;
  g.Hm = d->Hm; g.Wm = d->Wm; g.Hs = d->Hs; g.Ws = d->Ws; g.sm = d->sm; g.sd = d->sd;
  g.up2 = d->up2;
  if (d->up2) {      // the planar matrix's rows, from the side of the problem that walks them (GemmP::up2)
    const int rows = d->form == GEMM_TN ? d->K : d->M;
    const bool planar = d->up2 == 2 || (d->up2 == 1 && d->form == GEMM_NT);      // four planes of whole images + padding | the pixels themselves
    ARG_CHECK(d->Hm > 0 && d->Wm > 0, "gemm_route: up2 needs the image size");
    g.up_plane = planar ? rows / 4 : (int)upconv_plane_rows(1, 1, rows);
    g.up_rows = planar ? g.up_plane / (d->Hm * d->Wm) * (d->Hm * d->Wm) : rows;
  }
  g.geglu = d->geglu; g.geglu_group = d->geglu_group;
  if (d->geglu) { g.aux = (bf16*)word; g.ldaux = 8; }
  g.splitk = d->splitk; g.slab = word;
  if (d->group > 1) {
    g.group = d->group;
    for (int i = 0; i < d->group && i < GEMM_MAX_GROUP; ++i) { g.gA[i] = g.gB[i] = (const bf16*)word; g.gC[i] = word; g.gCb[i] = d->emit_bf16 ? (bf16*)word : nullptr; g.gbias_grad[i] = d->bias_grad ? word : nullptr; }
  } else if (d->emit_bf16) g.Cb = (bf16*)word;
  if (d->bias_grad) g.bias_grad = word;
  if (d->rowvec) { g.rowvec = (const bf16*)word; g.ldv = 8; g.rows_per_batch = d->M; }      // (one sample: no route looks at the sample height)
  if (d->delta) { g.delta_out = word; g.delta_o = (const bf16*)word; g.delta_nq = d->M; g.delta_heads = d->N / 64; }
  GemmRoute r;
  if (int e = gemm_route_checked(g, &r)) return e;
  out->kernel = r.kernel; out->cfg = r.cfg; out->fast = r.fast; out->post = r.post;
  return 0;
}
int sdxl_profile_gemm_begin(void) { return gemm_profile_begin(); }
int sdxl_set_gemm_mode(int mode) {
  const int cfg = mode >> 2;
  ARG_CHECK(mode >= 0 && (mode & 3) <= 2 && (cfg == 0 || cfg == 1 || cfg == 2 || cfg == 3 || cfg == 5 || cfg == 6 || cfg == 7 || cfg == 8 || cfg == 13 || cfg == 23 || cfg == 43 || cfg == 31 || cfg == 32 || cfg == 33 || cfg == 34 || cfg == 35 || cfg == 36), "gemm mode %d", mode);
  gemm_set_mode(mode);
  return 0;
}
int sdxl_profile_gemm_end(double* flops, double* ms, int* launches) { return gemm_profile_end(flops, ms, launches); }
#ifdef SDXL_DIAG     // ---- experiment ABI of the diagnostics build (include/sdxlstep_diag.h): not in the product library ----
// dY [M][Kr] x W [Kr][N] (the NN dgrad form) with the LayerNorm backward of GemmP::ln_x in the epilogue: dx = LN_bwd(dY W | x, stats, gamma)
// (+ addend), dy_out (or null) = dY W, pcol (or null) = [cdiv(M, 128)][2][N] dgamma | dbeta partial sums.  The granule scratch is the hooks'
// (the plan shares its own), zeroed on the stream before the launches; stream-ordered like every other hook.  N <= 1280.
int sdxl_op_linear_dgrad_ln_bwd(const void* dy, const void* w, const void* x, const float* stats, const void* gamma, const void* addend,
                                void* dx, void* dy_out, float* pcol, int M, int N, int Kr, void* st) {
  ARG_CHECK(gemm_ln_cfg(M, N, Kr) != 0, "linear_dgrad_ln_bwd: M=%d N=%d K=%d does not fit the fused epilogue", M, N, Kr);
  float* part;
  const size_t pbytes = gemm_ln_part_floats(M, N) * sizeof(float);
  CHK(hook_scratch(pbytes, (void**)&part));
  HIP_CHECK_RET(hipMemsetAsync(part, 0, pbytes, (hipStream_t)st));
  GemmP g = linear_dgrad_problem((const bf16*)dy, Kr, (const bf16*)w, dy_out, N, M, N, Kr, nullptr, 0);
  for (int epoch = 1; epoch <= 3; ++epoch) {      // three launches on the same scratch: later ones find the earlier epochs' granules
    gemm_attach_ln_bwd(g, (const bf16*)x, N, stats, (const bf16*)gamma, (bf16*)dx, (const bf16*)addend, part, epoch, pcol);
    CHK(launch_gemm(g, (hipStream_t)st));
  }
  return 0;
}
// Knobs are process-global and read at plan-build, forward and backward time: set them BEFORE sdxl_plan / the first step of a handle and
// leave them alone afterwards (A/B runs restart the process per setting, profiles/tools/ab.sh).
int sdxl_set_knob(int id, int value) {
  ARG_CHECK(id >= 0 && id < SDXL_NKNOBS, "knob %d out of range", id);
  g_knobs[id] = value;
  if (id == 9) wgrad256_set_enabled(value == 0);         // knob 9 = 1: long-reduction linear weight gradients on the 128 x 160 kernel
  if (id == 12) conv_wgrad3_set_enabled(value == 0);    // knob 12 = 1: 3x3 weight gradients on the one-tap-per-workgroup kernel only
  if (id == 15) gemm256_set_tail(value == 0);     // knob 15 = 1: no half-height tail workgroups in the 256 x 256 kernel
  return 0;
}
int sdxl_set_sk_mode(int mode, int workers) {
  ARG_CHECK(mode >= 0 && mode <= 2 && workers >= 0 && workers <= 256, "stream-K mode %d / workers %d", mode, workers);
  gemm_set_sk_mode(mode);
  gemm_sk_set_workers(workers);
  return 0;
}
int sdxl_op_pl_prefetch_b(int form, const void* B, int M, int N, int K, long ldb, int parts, void* st) {
  GemmP p;
  gemm_defaults(&p);
  p.form = form; p.B = (const bf16*)B; p.M = M; p.N = N; p.K = K; p.ldb = ldb;
  return launch_pl_prefetch_b(p, parts, (hipStream_t)st);
}
int sdxl_ln_error(unsigned* out) {
  ARG_CHECK(out != nullptr, "ln_error: null output");
  return gemm_ln_error(out);
}
int sdxl_sk_error(void* st, unsigned* out) {
  ARG_CHECK(out, "null output");
  return gemm_sk_error((hipStream_t)st, out);
}
int sdxl_op_gemm_sk(int n, const int* form, const void* const* A, const void* const* B, void* const* C, const int* M, const int* N,
                    const int* K, const void* const* bias, const void* const* resid, const int* accumulate, void* st) {
  ARG_CHECK(n >= 1 && n <= 4 && form && A && B && C && M && N && K, "gemm_sk: bad arguments");
  GemmP g[4];
  for (int i = 0; i < n; ++i) {
    CHK(dense_problem(form[i], A[i], B[i], C[i], M[i], N[i], K[i], bias ? bias[i] : nullptr, resid ? resid[i] : nullptr, accumulate ? accumulate[i] : 0, &g[i]));
  }
  return launch_gemm_multi(g, n, (hipStream_t)st);
}
#endif   // SDXL_DIAG

// debug: order-independent checksum (sum of raw 16-bit patterns) of every activation of the current plan, in
// creation order.  Synchronises.  Used to localise run-to-run differences.
__global__ void checksum_kernel(const unsigned short* __restrict__ x, long n, unsigned long long* out) {
  unsigned long long s = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    s += (unsigned long long)x[i] * (unsigned long long)((i % 251) + 1);
  atomicAdd(out, s);
}
int sdxl_debug_act_checksums(sdxl_handle* h, unsigned long long* out_host, int cap, int* n_out, int grads) {
  H_CHECK(h);
  CHK(ready(h->e));
  Plan& p = *h->e.cur;
  int n = (int)p.acts.size();
  if (n_out) *n_out = n;
  if (n > cap) n = cap;
  unsigned long long* d;
  HIP_CHECK_RET(hipDeviceSynchronize());      // the hooks' scratch is used on the null stream here: no hook of another stream may still be running on it
  CHK(hook_scratch(sizeof(unsigned long long) * (n > 0 ? n : 1), (void**)&d));
  HIP_CHECK_RET(hipMemset(d, 0, sizeof(unsigned long long) * (n > 0 ? n : 1)));
  for (int i = 0; i < n; ++i) {
    Act* a = p.acts[i].get();
    const bf16* src = grads ? p.G(a) : p.P(a);
    if (!src || a->parent) continue;     // (column-slice views are covered by their parent)
    long cnt = a->rows * a->cols;
    hipLaunchKernelGGL(checksum_kernel, dim3(64), dim3(256), 0, 0, (const unsigned short*)src, cnt, d + i);
  }
  HIP_CHECK_RET(hipDeviceSynchronize());
  HIP_CHECK_RET(hipMemcpy(out_host, d, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

// ---- LoKr on caller buffers (csrc/lokr.hip; the hook is a dtype, SDXL_DTYPE_LOKR_ONE, so nothing here is exported): the descriptor of one target,
// every offset 0; the form and the scale are the caller's choice, not the rule's ----
static int lokr_one(int out, int in, int group, int kind, int factor, int rank, int full, float scale, LokrP& q) {
  CHK(lokr_check_fields(rank, factor, full));
  LoraP l;
  CHK(lora_one_layout(out, in, rank, scale, kind, group, out, l));
  memset(&q, 0, sizeof(q));
  q.n = 1; q.rank = rank; q.scale = q.scale_full = scale;
  q.one.t = l.one;
  lokr_geometry(q.one, kind == LORA_KIND_CONV3 ? group : in, factor, full);
  CHK(lokr_check_size("the operand", q.one, rank));
  q.one.part_off = 0; q.one.dw2_off = (long)lokr_part_floats(q.one);
  q.tiles_m = lokr_tiles_m(q.one); q.tiles_p = q.one.ptiles; q.tiles_q = lokr_tiles_q(q.one, rank);
  return 0;
}
// the two halves of SDXL_DTYPE_LOKR_ONE (sdxlstep_diag.h): no symbol of their own, capi.hip's sdxl_load_weight / sdxl_export_grad call them
int lokr_one_merge(const sdxl_lokr_one* o, void* st) {
  ARG_CHECK(o != nullptr, "lokr_merge: NULL descriptor");
  ARG_CHECK(aligned16(o->base) && aligned16(o->C) && aligned16(o->W2) && (o->full == 1 || aligned16(o->A)) && aligned16(o->w),
            "lokr_merge: every pointer must be 16-byte aligned and non-NULL");
  LokrP q;
  CHK(lokr_one(o->out, o->in, o->group, o->kind, o->factor, o->rank, o->full, o->scale, q));
  q.w = (bf16*)o->w; q.base = (const bf16*)o->base;
  q.c = (const bf16*)o->C; q.b = (const bf16*)o->W2; q.a = (const bf16*)o->A;
  return launch_lokr_merge(q, (hipStream_t)st);
}
int lokr_one_project(const sdxl_lokr_one* o, void* st) {
  ARG_CHECK(o != nullptr, "lokr_project: NULL descriptor");
  ARG_CHECK(aligned16(o->dw) && aligned16(o->C) && aligned16(o->W2) && aligned16(o->dC) && aligned16(o->dW2) &&
            (o->full == 1 || (aligned16(o->A) && aligned16(o->dA))), "lokr_project: every pointer must be 16-byte aligned and non-NULL");
  LokrP q;
  CHK(lokr_one(o->out, o->in, o->group, o->kind, o->factor, o->rank, o->full, o->scale, q));
  CHK(lokr_check_scratch(o->scratch, o->scratch_floats, lokr_part_floats(q.one) + lokr_dw2_floats(q.one)));
  q.dw = o->dw; q.c = (const bf16*)o->C; q.b = (const bf16*)o->W2; q.a = (const bf16*)o->A;
  q.gc = o->dC; q.gb = o->dW2; q.ga = o->dA; q.scratch = o->scratch;
  return launch_lokr_project(q, (hipStream_t)st);
}

// ---- DoRA on caller buffers (csrc/dora.hip; the hook is a dtype, SDXL_DTYPE_DORA_ONE, so nothing here is exported): the descriptor of one
// target, every offset 0 ----
static int dora_one(const sdxl_dora_one* o, int mode, DoraP& q) {
  CHK(dora_check_fields(o->rank, mode));
  LoraP l;
  CHK(lora_one_layout(o->out, o->in, o->rank, o->scale, o->kind, o->group, o->out, l));
  memset(&q, 0, sizeof(q));
  q.n = 1; q.rank = o->rank; q.scale = o->scale; q.mapped = 1;
  q.one.t = l.one;
  q.tiles_m = l.tiles_m; q.tiles_b = l.tiles_b; q.tiles_a = l.tiles_a;
  q.base = (const bf16*)o->base; q.a = (const bf16*)o->A; q.b = (const bf16*)o->B; q.mu = (const bf16*)o->mu; q.w = (bf16*)o->w;
  q.dw = o->dw; q.ga = o->dA; q.gb = o->dB; q.gmu = o->dmu; q.norm0 = o->norm0; q.norm = o->norm;
  return 0;
}
// the two halves of SDXL_DTYPE_DORA_ONE (sdxlstep_diag.h): no symbol of their own, capi.hip's sdxl_load_weight / sdxl_export_grad call them
int dora_one_load(const sdxl_dora_one* o, void* st) {
  ARG_CHECK(o != nullptr, "dora_load: NULL descriptor");
  CHK(dora_check_fields(o->rank, o->mode));
  ARG_CHECK(aligned16(o->base) && (o->mode == 1 || aligned16(o->w)) && (o->mode == 2 || aligned16(o->norm0)) &&
            (o->mode != 0 || (aligned16(o->A) && aligned16(o->B) && aligned16(o->mu) && aligned16(o->norm))),
            "dora_load: every pointer the mode uses must be 16-byte aligned and non-NULL");
  DoraP q;
  CHK(dora_one(o, o->mode, q));
  return o->mode == 0 ? launch_dora_merge(q, (hipStream_t)st) : o->mode == 1 ? launch_dora_init(q, (hipStream_t)st) : launch_dora_restore(q, (hipStream_t)st);
}
int dora_one_project(const sdxl_dora_one* o, void* st) {
  ARG_CHECK(o != nullptr, "dora_project: NULL descriptor");
  ARG_CHECK(aligned16(o->dw) && aligned16(o->base) && aligned16(o->A) && aligned16(o->B) && aligned16(o->mu) && aligned16(o->norm0) &&
            aligned16(o->norm) && aligned16(o->dA) && aligned16(o->dB) && aligned16(o->dmu),
            "dora_project: every pointer must be 16-byte aligned and non-NULL");
  DoraP q;
  CHK(dora_one(o, 0, q));
  return launch_dora_project(q, (hipStream_t)st);
}
