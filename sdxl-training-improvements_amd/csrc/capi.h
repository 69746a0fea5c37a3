// What the two halves of the extern "C" surface share: the handle, and the checks / fills that a product entry point (capi.hip) and its
// single-kernel hook (hooks.hip) both go through.  Included by those two files only.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include "engine.h"
#include "../../include/sdxlstep_diag.h"

const char* sdxl_get_error();

struct StepState {  // what backward needs from the preceding forward
  sdxl_loss_config lc;      // in full (read_loss_config), the flag cleared
  sdxl_batch b;
  bool valid = false;
  float* d_ehs = nullptr;   // the conditioning gradients this micro-step asked for (sdxl_batch_ext): the caller's
  float* d_pool = nullptr;  // buffers, written behind the backward from the plan's
  bool awaiting_bwd = false;   // a sdxl_forward_loss whose backward has not finished: the gradient selection may not change under it
  ResidualReq res;             // the additional skip residuals this micro-step carried (sdxl_batch_res): the backward writes res.d_*
  float* d_input = nullptr;    // the input gradient this micro-step asked for (sdxl_batch_din): the caller's buffer, written by conv_in's backward
};
struct LoraCache {  // device table of the last SDXL_DTYPE_LORA / SDXL_DTYPE_LORA_LAYOUTS / SDXL_DTYPE_LOHA / SDXL_DTYPE_LOKR / SDXL_DTYPE_DORA call
  void* dev = nullptr;          // LoraTarget, LohaTarget, LokrTarget or DoraTarget [params.size()]: `dtype` says which
  int dtype = 0, rank = 0;      // the key: (dtype, rank, target list, factor, full); factor and full are 0 but for SDXL_DTYPE_LOKR
  std::vector<int> params;
  int factor = 0, full = 0;
  int mapped = 0;
  size_t scratch_floats = 0;    // what SDXL_DTYPE_LOKR's projection needs of sdxl_lokr_op.scratch
  int tiles_m = 0, tiles_b = 0, tiles_a = 0;
};
// whoever builds a table frees the cached one first (hipFree waits for the launches that read it)
static void lora_cache_free(LoraCache& c) {
  if (c.dev) { (void)hipFree(c.dev); c.dev = nullptr; }
}
struct sdxl_handle {
  Engine e;
  StepState step;
  LoraCache lora;
};

#define H_CHECK(h) ARG_CHECK((h) != nullptr, "null handle")
#define CHK(x)         \
  do {                 \
    int _r = (x);      \
    if (_r) return _r; \
  } while (0)

// the shape check every LoRA entry point shares, and the alignment its pointers need
static int lora_check_shape(const char* who, int out, int in, int rank) {
  ARG_CHECK(rank >= 1 && rank <= 128, "lora: rank %d outside 1 .. 128", rank);
  ARG_CHECK(out >= 1 && in >= 8 && in % 8 == 0, "lora: '%s' is [%d][%d]: `in` must be a positive multiple of 8 (16-byte rows)", who, out, in);
  return 0;
}
static bool aligned16(const void* p) { return p && ((uintptr_t)p & 15) == 0; }
// ... and of every LoHa entry point (SDXL_DTYPE_LOHA, the sdxl_op_loha_* hooks): the effective rank is rank^2, so the cap is lower
static int loha_check_rank(int rank) {
  ARG_CHECK(rank >= 1 && rank <= LOHA_MAX_RANK, "loha: rank %d outside 1 .. %d", rank, LOHA_MAX_RANK);
  return 0;
}

// ... and of every LoKr entry point (SDXL_DTYPE_LOKR, the hook SDXL_DTYPE_LOKR_ONE)
static int lokr_check_fields(int rank, int factor, int full) {
  ARG_CHECK(rank >= 1 && rank <= LOKR_MAX_RANK, "lokr: rank %d outside 1 .. %d", rank, LOKR_MAX_RANK);
  ARG_CHECK(factor == -1 || factor >= 1, "lokr: factor %d (-1, or a positive integer)", factor);
  ARG_CHECK(full == 0 || full == 1, "lokr: full %d (0 or 1)", full);
  return 0;
}
// the projection indexes W2, B, A and their tiles with 32-bit integers
static int lokr_check_size(const char* who, const LokrTarget& x, int rank) {
  const long lim = (1L << 31) - 2 * LOKR_P_TILE;
  ARG_CHECK((long)x.out_k * x.n2 < lim && (long)x.out_k * rank < lim && (long)rank * x.n2 < lim,
            "lokr: '%s' has a second factor of %d x %d elements at rank %d: too large", who, x.out_k, x.n2, rank);
  return 0;
}
static int lokr_check_scratch(const float* scratch, size_t have, size_t need) {
  ARG_CHECK(aligned16(scratch), "lokr: scratch must be a 16-byte aligned device pointer");
  ARG_CHECK(have >= need, "lokr: scratch holds %zu floats, the projection of these targets needs %zu", have, need);
  return 0;
}
// SDXL_DTYPE_LOKR_ONE (hooks.hip): one target on caller buffers, no handle
int lokr_one_merge(const sdxl_lokr_one* o, void* st);
int lokr_one_project(const sdxl_lokr_one* o, void* st);
static_assert(LOKR_P_TILE == SDXL_LOKR_TILE, "the scratch formula of include/sdxlstep.h");

// ... and of every DoRA entry point (SDXL_DTYPE_DORA, the hook SDXL_DTYPE_DORA_ONE)
static int dora_check_fields(int rank, int mode) {
  ARG_CHECK(rank >= 1 && rank <= 128, "dora: rank %d outside 1 .. 128", rank);
  ARG_CHECK(mode >= 0 && mode <= 2, "dora: mode %d (0 merge, 1 init, 2 restore)", mode);
  return 0;
}
static int dora_check_norms(const float* norm0, const float* norm) {
  ARG_CHECK(aligned16(norm0), "dora: norm0 must be a 16-byte aligned device pointer");
  ARG_CHECK(aligned16(norm), "dora: norm must be a 16-byte aligned device pointer");
  return 0;
}
// SDXL_DTYPE_DORA_ONE (hooks.hip): one target on caller buffers, no handle
int dora_one_load(const sdxl_dora_one* o, void* st);
int dora_one_project(const sdxl_dora_one* o, void* st);
static_assert(DORA_R_ROWS == LORA_B_ROWS, "the row reductions share LoraTarget::tile_b with dB");

// a handle that can run a step: planned, bound, with its workspace
static int ready(Engine& e) {
  if (!e.cur) { sdxl_set_error("no plan: call sdxl_plan first"); return 3; }
  if (!e.weights || !e.grads) { sdxl_set_error("parameters are not bound: call sdxl_bind_params"); return 3; }
  if (!e.ws || e.ws_cap < e.cur->ws_bytes) {
    sdxl_set_error("workspace too small: have %zu bytes, plan needs %zu", e.ws_cap, e.cur->ws_bytes);
    return 3;
  }
  return 0;
}

// The caller's sdxl_loss_config is the short struct (everything before mask_norm) unless loss_type carries SDXL_LOSS_EXT: this is the
// one place that reads it.  `out` is the struct in full with the flag cleared (loss_type = the element loss) and the fields the caller
// did not pass zero / NULL; every other function here takes that copy.  loss_type's own errors come before any appended field is read.
static int read_loss_config(const sdxl_loss_config* lc, sdxl_loss_config* out) {
  const int lt = lc->loss_type;
  ARG_CHECK(lt >= 0 && (lt & 0xff) <= 2 && (lt & ~(0xff | SDXL_LOSS_EXT)) == 0,
            "loss_type %d (0 = l2, 1 = huber, 2 = smooth_l1, optionally | SDXL_LOSS_EXT)", lt);
  memset(out, 0, sizeof(*out));
  memcpy(out, lc, (lt & SDXL_LOSS_EXT) ? sizeof(*out) : offsetof(sdxl_loss_config, mask_norm));
  out->loss_type = lt & 0xff;
  ARG_CHECK(!out->loss_mask || (out->mask_norm >= 0 && out->mask_norm <= 1), "mask_norm %d (0 = mean, 1 = masked_mean)", out->mask_norm);
  if (!out->loss_mask) out->mask_norm = 0;      // read only with a mask
  return 0;
}
// the appended fields of sdxl_loss_config / sdxl_batch (element loss, per-sample weights / c / losses, mask, the input's noise), for
// both places that fill a LossP; lc is read_loss_config's copy
static void fill_loss_ext(const sdxl_loss_config* lc, const sdxl_batch* b, LossP& L) {
  L.loss_type = lc->loss_type; L.huber_c = lc->huber_c;
  L.sample_w = b->sample_weights; L.huber_cb = b->huber_c; L.ps_out = b->per_sample_loss;
  L.mask = lc->loss_mask; L.mask_norm = lc->mask_norm;
  L.noise_in = lc->noise_in ? lc->noise_in : b->noise;
}
// ... and their argument errors, reported before anything is copied or launched
static int check_loss_ext(const sdxl_loss_config* lc, const sdxl_batch* b) {
  ARG_CHECK(lc->loss_type == 0 || b->huber_c || lc->huber_c > 0.f, "loss_type %d needs huber_c > 0 (got %g) or a per-sample huber_c array",
            lc->loss_type, (double)lc->huber_c);
  return 0;
}

// sdxl_batch_cond's two fields (extra UNet input channels), read only behind SDXL_BATCH_COND: a caller without the flag passes a shorter
// struct.  SDXL_BATCH_FLAGS: what the flags leave of ctx_len; either flag says that sdxl_batch_ext's fields are there.
#define SDXL_BATCH_FLAGS (SDXL_BATCH_EXT | SDXL_BATCH_COND | SDXL_BATCH_RES | SDXL_BATCH_DIN)
static void read_input_cond(const sdxl_batch* b, const float** cond, int* channels) {
  *cond = nullptr; *channels = 0;
  if (!(b->ctx_len & (SDXL_BATCH_COND | SDXL_BATCH_RES | SDXL_BATCH_DIN))) return;      // (sdxl_batch_res / sdxl_batch_din hold a sdxl_batch_cond in full)
  const sdxl_batch_cond* x = (const sdxl_batch_cond*)b;
  *cond = x->input_cond; *channels = x->cond_channels;
}
// sdxl_batch_res's one field (additional skip residuals), read only behind SDXL_BATCH_RES, with its argument errors -- reported before
// anything is copied or launched.  `out` is a copy of the caller's host arrays (they are read during the call only); nskip = the handle's
// number of skips.  Without the flag or with a NULL pointer: out->present is false and nothing else of it is looked at.
static int read_residuals(const sdxl_batch* b, int nskip, ResidualReq* out) {
  *out = ResidualReq();
  if (!b || !(b->ctx_len & (SDXL_BATCH_RES | SDXL_BATCH_DIN))) return 0;      // (sdxl_batch_din holds a sdxl_batch_res in full)
  const sdxl_residuals* r = ((const sdxl_batch_res*)b)->residuals;
  if (!r) return 0;
  ARG_CHECK(r->n == nskip, "residuals: n = %d, the UNet saves %d skips (1 + 3 * layers_per_block + 2)", r->n, nskip);
  ARG_CHECK(r->dtype == 0 || r->dtype == 1, "residuals: dtype %d (0 = fp32, 1 = bf16)", r->dtype);
  for (int i = 0; i < nskip; ++i) {
    ARG_CHECK(!r->down || ((uintptr_t)r->down[i] & 15) == 0, "residuals: down[%d] is not 16-byte aligned", i);
    ARG_CHECK(!r->d_down || ((uintptr_t)r->d_down[i] & 15) == 0, "residuals: d_down[%d] is not 16-byte aligned", i);
  }
  ARG_CHECK(((uintptr_t)r->mid & 15) == 0, "residuals: mid is not 16-byte aligned");
  ARG_CHECK(((uintptr_t)r->d_mid & 15) == 0, "residuals: d_mid is not 16-byte aligned");
  out->present = true; out->dtype = r->dtype; out->mid = r->mid; out->d_mid = r->d_mid;
  if (r->down) out->down.assign(r->down, r->down + nskip);
  if (r->d_down) out->d_down.assign(r->d_down, r->d_down + nskip);
  if (b->sampler) {
    for (int i = 0; i < nskip; ++i) ARG_CHECK(!r->d_down || !r->d_down[i], "residuals: d_down[%d] cannot be combined with a sampler step", i);
    ARG_CHECK(!r->d_mid, "residuals: d_mid cannot be combined with a sampler step");
  }
  return 0;
}

// sdxl_batch_din's one field (the input gradient's output), read only behind SDXL_BATCH_DIN, with its argument errors -- reported before
// anything is copied or launched.  conv_in_cout: the width of conv_in's output (input_dgrad.hip reduces it in steps of 32).
static int read_input_grad(const sdxl_batch* b, int conv_in_cout, float** d_input) {
  *d_input = nullptr;
  if (!b || !(b->ctx_len & SDXL_BATCH_DIN)) return 0;
  float* d = ((const sdxl_batch_din*)b)->d_input;
  if (!d) return 0;
  ARG_CHECK(!b->sampler, "d_input cannot be combined with a sampler step");
  ARG_CHECK(((uintptr_t)d & 15) == 0, "d_input is not 16-byte aligned");
  ARG_CHECK(conv_in_cout % 32 == 0, "d_input: conv_in's output width %d is not a multiple of 32", conv_in_cout);
  *d_input = d;
  return 0;
}

// sdxl_sampler_step's argument errors (reported before anything is copied or launched) and its kernel parameters.  The caller's struct
// ends at guidance_rescale unless init carries SDXL_SAMPLER_EXT: nothing behind it is read without the flag.
static int fill_sampler(const sdxl_sampler_step* s, int image_batch, int HW, SamplerP& q) {
  ARG_CHECK(s->x != nullptr, "sampler: x is NULL");
  ARG_CHECK(!s->cfg || image_batch % 2 == 0, "sampler: cfg needs an even batch [cond; uncond] (got %d)", image_batch);
  const float v[8] = {s->a_skip, s->a_out, s->p, s->q, s->a_in_next, s->clamp, s->guidance, s->guidance_rescale};
  for (int i = 0; i < 8; ++i) ARG_CHECK(isfinite(v[i]), "sampler: scalar %d of (a_skip, a_out, p, q, a_in_next, clamp, guidance, guidance_rescale) is not finite", i);
  ARG_CHECK((s->init & ~(1 | SDXL_SAMPLER_EXT)) == 0, "sampler: init %d (0 | 1, optionally | SDXL_SAMPLER_EXT)", s->init);
  memset(&q, 0, sizeof(q));
  q.x = s->x;
  q.B = s->cfg ? image_batch / 2 : image_batch; q.HW = HW;
  q.cfg = s->cfg != 0; q.init = (s->init & 1) != 0;
  q.a_skip = s->a_skip; q.a_out = s->a_out; q.p = s->p; q.q = s->q; q.a_in_next = s->a_in_next; q.clamp = s->clamp;
  q.guidance = s->guidance; q.rescale = s->guidance_rescale;
  if (!(s->init & SDXL_SAMPLER_EXT)) return 0;
  const sdxl_sampler_step_ext* e = (const sdxl_sampler_step_ext*)s;
  const float w[5] = {e->r, e->u, e->s, e->k_a, e->k_b};
  for (int i = 0; i < 5; ++i) ARG_CHECK(isfinite(w[i]), "sampler: scalar %d of (r, u, s, k_a, k_b) is not finite", i);
  ARG_CHECK(e->save >= 0 && e->save <= 3, "sampler: save %d (bit 0: hist, bit 1: xsave)", e->save);
  ARG_CHECK(e->hist || (e->r == 0.f && !(e->save & 1)), "sampler: hist is NULL but r != 0 or save bit 0 is set");
  ARG_CHECK(e->xsave || (e->u == 0.f && !(e->save & 2)), "sampler: xsave is NULL but u != 0 or save bit 1 is set");
  ARG_CHECK(e->noise || e->s == 0.f, "sampler: noise is NULL but s != 0");
  ARG_CHECK(!e->mask || e->known, "sampler: mask needs known");
  ARG_CHECK(e->knoise || e->k_b == 0.f, "sampler: knoise is NULL but k_b != 0");
  q.ext = 1;
  q.hist = e->hist; q.xsave = e->xsave; q.noise = e->noise; q.r = e->r; q.u = e->u; q.s = e->s; q.save = e->save;
  q.mask = e->mask; q.known = e->known; q.knoise = e->knoise; q.k_a = e->k_a; q.k_b = e->k_b;
  return 0;
}
