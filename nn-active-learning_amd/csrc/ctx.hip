// Everything behind the C ABI that needs no model: the error text, contexts and their streams, launch profiling, and the
// pass-through entry points (top-k, masks, optimiser steps, loss statistics, gather / normalise, committee, evaluation counts, synth).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>

#include "alq_internal.h"

namespace alq {

static thread_local char g_err[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int loss_check(const char *who, const float *d_post_or_x, int c, const int32_t *d_labels, const alq_loss_t *loss) {
    ALQ_REQUIRE(d_post_or_x && loss, ALQ_EINVAL, "%s: null argument", who);
    ALQ_REQUIRE(c >= 1, ALQ_EINVAL, "%s: %d classes", who, c);
    ALQ_REQUIRE(loss->kind == ALQ_LOSS_CE || loss->kind == ALQ_LOSS_CE_SOFT || loss->kind == ALQ_LOSS_GCE, ALQ_EINVAL,
                "%s: loss kind %d", who, (int)loss->kind);
    ALQ_REQUIRE(loss->kind != ALQ_LOSS_CE || d_labels, ALQ_EINVAL, "%s: cross-entropy needs labels", who);
    ALQ_REQUIRE(loss->kind == ALQ_LOSS_CE || loss->d_targets, ALQ_EINVAL, "%s: CE_softclasses / GCE need targets", who);
    ALQ_REQUIRE(loss->kind != ALQ_LOSS_GCE || loss->gce_q != 0.f, ALQ_EINVAL, "%s: GCE with q = 0", who);
    ALQ_REQUIRE(!loss->d_old_logits || loss->lwf_T > 0.f, ALQ_EINVAL, "%s: LwF temperature %g", who, (double)loss->lwf_T);
    return ALQ_OK;
}

int flag_clear(alq_ctx *ctx) {
    ALQ_HIP(hipMemsetAsync(flag_of(ctx), 0, sizeof(int), ctx->stream));
    return ALQ_OK;
}

int flag_read(alq_ctx *ctx, int *bad) {
    ALQ_HIP(hipMemcpyAsync(bad, flag_of(ctx), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ALQ_HIP(hipStreamSynchronize(ctx->stream));
    return ALQ_OK;
}

}  // namespace alq

using namespace alq;

int alq_ctx::prof_begin(int cls, hipEvent_t *e0, hipEvent_t *e1) {
    ProfSlot &s = prof[cls];
    auto get = [&](hipEvent_t *ev) -> int {
        if (!s.pool.empty()) {
            *ev = s.pool.back();
            s.pool.pop_back();
            return ALQ_OK;
        }
        return hipEventCreate(ev) == hipSuccess ? ALQ_OK : ALQ_EHIP;
    };
    if (get(e0) != ALQ_OK || get(e1) != ALQ_OK) return ALQ_EHIP;
    return hipEventRecord(*e0, stream) == hipSuccess ? ALQ_OK : ALQ_EHIP;
}

void alq_ctx::prof_end(int cls, hipEvent_t e0, hipEvent_t e1, double flops) {
    ProfSlot &s = prof[cls];
    (void)hipEventRecord(e1, stream);
    s.pending.emplace_back(e0, e1);
    s.launches += 1;
    s.flops += flops;
}

int alq_ctx::prof_collect() {
    ALQ_HIP(hipStreamSynchronize(stream));
    for (int c = 0; c < PROF_NUM; ++c) {
        ProfSlot &s = prof[c];
        for (auto &pr : s.pending) {
            float ms = 0.f;
            ALQ_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
            s.ms += ms;
            s.pool.push_back(pr.first);
            s.pool.push_back(pr.second);
        }
        s.pending.clear();
    }
    return ALQ_OK;
}

// =========================================================================================== C ABI
extern "C" {

const char *alq_last_error(void) { return g_err; }
int alq_version(void) { return 1; }

int alq_ctx_create(int device, void *stream, alq_ctx **out) {
    ALQ_REQUIRE(out != nullptr, ALQ_EINVAL, "alq_ctx_create: null out");
    int count = 0;
    ALQ_HIP(hipGetDeviceCount(&count));
    ALQ_REQUIRE(device >= 0 && device < count, ALQ_EINVAL, "device %d not present (%d visible)", device, count);
    ALQ_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ALQ_HIP(hipGetDeviceProperties(&prop, device));
    ALQ_REQUIRE(std::strncmp(prop.gcnArchName, "gfx950", 6) == 0, ALQ_EUNSUPPORTED,
                "libalq is built for gfx950 (MI355X) only, device %d is %s", device, prop.gcnArchName);
    alq_ctx *c = new alq_ctx();
    c->device = device;
    if (prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    c->stream = reinterpret_cast<hipStream_t>(stream);
    if (hipMalloc(&c->param_block, ALQ_PARAM_BLOCK_BYTES) != hipSuccess) {
        delete c;
        set_error("alq_ctx_create: hipMalloc failed");
        return ALQ_ENOMEM;
    }
    if (!std::getenv("ALQ_NO_SIDE_STREAM")) {      // diagnostic: everything on one stream
        if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (c->side) (void)hipStreamDestroy(c->side);
            if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
            c->side = nullptr; c->ev_fork = nullptr; c->ev_join = nullptr;
        }
    }
    *out = c;
    return ALQ_OK;
}

int alq_ctx_destroy(alq_ctx *ctx) {
    if (!ctx) return ALQ_OK;
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) {
        (void)hipStreamSynchronize(ctx->side);
        (void)hipStreamDestroy(ctx->side);
        (void)hipEventDestroy(ctx->ev_fork);
        (void)hipEventDestroy(ctx->ev_join);
    }
    (void)alq_comm_destroy(ctx);
    for (int c = 0; c < PROF_NUM; ++c) {
        for (auto &pr : ctx->prof[c].pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (auto e : ctx->prof[c].pool) (void)hipEventDestroy(e);
    }
    (void)hipFree(ctx->param_block);
    if (ctx->loss_part) (void)hipFree(ctx->loss_part);
    if (ctx->mt_part) (void)hipFree(ctx->mt_part);
    if (ctx->sq_part) (void)hipFree(ctx->sq_part);
    for (void *p : ctx->sq_retired) (void)hipFree(p);
    delete ctx;
    return ALQ_OK;
}

int alq_ctx_use_side_stream(alq_ctx *ctx, int on) {
    ALQ_REQUIRE(ctx != nullptr, ALQ_EINVAL, "null ctx");
    ctx->side_off = on == 0;
    return ALQ_OK;
}

int alq_ctx_set_stream(alq_ctx *ctx, void *stream) {
    ALQ_REQUIRE(ctx != nullptr, ALQ_EINVAL, "null ctx");
    hipStream_t next = reinterpret_cast<hipStream_t>(stream);
    if (next != ctx->stream) {
        // the library's hidden state (activation workspaces, partial sums, side-stream work joined into the OLD stream) is
        // ordered on the old stream only: the new stream waits for everything enqueued there so far
        ALQ_HIP(hipSetDevice(ctx->device));
        hipEvent_t ev;
        ALQ_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e1 = hipEventRecord(ev, ctx->stream);
        hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(next, ev, 0) : e1;
        (void)hipEventDestroy(ev);
        ALQ_REQUIRE(e2 == hipSuccess, ALQ_EHIP, "alq_ctx_set_stream: %s", hipGetErrorString(e2));
        ctx->stream = next;
    }
    return ALQ_OK;
}

int alq_ctx_synchronize(alq_ctx *ctx) {
    ALQ_REQUIRE(ctx != nullptr, ALQ_EINVAL, "null ctx");
    ALQ_HIP(hipStreamSynchronize(ctx->stream));
    return ALQ_OK;
}

static const char *kProfNames[PROF_NUM] = {"igemm_fwd", "igemm_bwd", "elementwise", "reduce", "fc_small",
                                           "igemm3_fwd", "igemm3_bwd", "direct_conv", "igemm_f16x2", "gnorm",
                                           "committee", "eval"};

int alq_prof_enable(alq_ctx *ctx, int on) {
    ALQ_REQUIRE(ctx != nullptr, ALQ_EINVAL, "null ctx");
    ctx->prof_on = on != 0;
    ctx->prof_every = on > 1 ? on : 1;
    ctx->prof_pass = 0;
    return ALQ_OK;
}

int alq_prof_reset(alq_ctx *ctx) {
    ALQ_REQUIRE(ctx != nullptr, ALQ_EINVAL, "null ctx");
    ALQ_TRY(ctx->prof_collect());
    for (int c = 0; c < PROF_NUM; ++c) {
        ctx->prof[c].ms = 0; ctx->prof[c].launches = 0; ctx->prof[c].flops = 0;
    }
    return ALQ_OK;
}

int alq_prof_num_classes(void) { return PROF_NUM; }
const char *alq_prof_class_name(int cls) { return (cls >= 0 && cls < PROF_NUM) ? kProfNames[cls] : ""; }

int alq_prof_read(alq_ctx *ctx, int cls, double *ms, int64_t *launches, double *flops) {
    ALQ_REQUIRE(ctx && cls >= 0 && cls < PROF_NUM, ALQ_EINVAL, "alq_prof_read: bad class");
    ALQ_TRY(ctx->prof_collect());
    if (ms) *ms = ctx->prof[cls].ms;
    if (launches) *launches = ctx->prof[cls].launches;
    if (flops) *flops = ctx->prof[cls].flops;
    return ALQ_OK;
}

int alq_gather_normalize(alq_ctx *ctx, const void *const *d_vols, int mm, int vol_is_f64,
                         const int64_t pad_dims[3], const int64_t *d_inds, int64_t n,
                         const int32_t ps[3], const double *h_stats, int quirk, int out_is_f64, void *d_out) {
    ALQ_REQUIRE(ctx && d_vols && pad_dims && ps && d_out && (n == 0 || d_inds), ALQ_EINVAL, "alq_gather_normalize: null argument");
    ALQ_REQUIRE(mm >= 1 && mm <= 16, ALQ_EINVAL, "alq_gather_normalize: %d modalities", mm);
    ALQ_REQUIRE(quirk == 2 || h_stats, ALQ_EINVAL, "alq_gather_normalize: stats missing");
    if (n == 0) return ALQ_OK;
    int64_t orig[3];
    for (int d = 0; d < 3; ++d) {
        ALQ_REQUIRE(ps[d] >= 1 && (ps[d] & 1), ALQ_EINVAL, "patch dims must be odd (patch_utils.py:1119-1121), got %d", ps[d]);
        orig[d] = pad_dims[d] - 2 * ((ps[d] - 1) / 2);
        ALQ_REQUIRE(orig[d] >= 1, ALQ_EINVAL, "padded volume smaller than the patch");
    }
    ALQ_HIP(hipSetDevice(ctx->device));
    // small device-side parameter block: m pointers + 2m doubles
    struct Block { const void *ptrs[16]; double stats[32]; } hb;
    std::memset(&hb, 0, sizeof(hb));
    for (int j = 0; j < mm; ++j) {
        hb.ptrs[j] = d_vols[j];
        if (h_stats) { hb.stats[2 * j] = h_stats[2 * j]; hb.stats[2 * j + 1] = h_stats[2 * j + 1]; }
    }
    static_assert(sizeof(Block) <= ALQ_PARAM_FLAG_OFFSET, "parameter block too small");
    Block *db = reinterpret_cast<Block *>(ctx->param_block);
    // pageable source: the copy is staged before the call returns, and it is stream-ordered
    // behind any kernel of an earlier call that still reads the block
    ALQ_HIP(hipMemcpyAsync(db, &hb, sizeof(Block), hipMemcpyHostToDevice, ctx->stream));
    return gather_normalize_impl(ctx, db->ptrs, mm, vol_is_f64, pad_dims, orig, d_inds, n, ps, db->stats, quirk,
                                 out_is_f64, d_out);
}

int alq_score_entropy(alq_ctx *ctx, const float *d_p1, int64_t n, double *d_absdev, float *d_H) {
    ALQ_REQUIRE(ctx && (n == 0 || d_p1), ALQ_EINVAL, "alq_score_entropy: null argument");
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    return score_entropy_impl(ctx, d_p1, n, d_absdev, d_H);
}

int alq_committee_update(alq_ctx *ctx, const float *d_p1, int64_t n, int member, int mode, double *d_mean_p, double *d_mean_h,
                         double *d_keys) {
    ALQ_REQUIRE(ctx && n >= 0 && member >= 0, ALQ_EINVAL, "alq_committee_update: bad argument (n=%lld member=%d)", (long long)n,
                member);
    ALQ_REQUIRE(mode == ALQ_COMMITTEE_ENSEMBLE || mode == ALQ_COMMITTEE_QBC_JS, ALQ_EINVAL, "alq_committee_update: mode %d", mode);
    ALQ_REQUIRE(n == 0 || (d_p1 && d_mean_p && (mode == ALQ_COMMITTEE_ENSEMBLE || d_mean_h)), ALQ_EINVAL,
                "alq_committee_update: null argument");
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    return committee_update_impl(ctx, d_p1, n, member, mode, d_mean_p, d_mean_h, d_keys);
}

int alq_eval_counts(alq_ctx *ctx, const int64_t *d_pred, const int64_t *d_inds, int64_t n, const void *d_mask, int mask_is_f64,
                    int64_t mask_elems, int64_t *d_counts, uint8_t *d_seg) {
    ALQ_REQUIRE(ctx && n >= 0 && mask_elems >= 0, ALQ_EINVAL, "alq_eval_counts: bad argument (n=%lld mask_elems=%lld)", (long long)n,
                (long long)mask_elems);
    ALQ_REQUIRE(n == 0 || (d_pred && d_mask && d_counts), ALQ_EINVAL, "alq_eval_counts: null argument");
    ALQ_REQUIRE(d_inds || n <= mask_elems, ALQ_EINVAL, "alq_eval_counts: %lld samples, a label vector of %lld", (long long)n,
                (long long)mask_elems);
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    if (d_inds) ALQ_TRY(flag_clear(ctx));
    ALQ_TRY(eval_counts_impl(ctx, d_pred, d_inds, n, d_mask, mask_is_f64, mask_elems, d_counts, d_seg, flag_of(ctx)));
    if (d_inds) {
        // the indices live on the device: the kernel skipped any outside the volume and raised the flag
        int bad = 0;
        ALQ_TRY(flag_read(ctx, &bad));
        ALQ_REQUIRE(!bad, ALQ_EINVAL, "alq_eval_counts: an index outside [0, %lld)", (long long)mask_elems);
    }
    return ALQ_OK;
}

size_t alq_topk_work_bytes(int64_t n) { return topk_work_bytes_impl(n); }

int alq_topk_uncertain(alq_ctx *ctx, const double *d_keys, int64_t n, int64_t B, int64_t *d_out_idx, void *d_work) {
    ALQ_REQUIRE(ctx && (n == 0 || (d_keys && d_work)) && (B == 0 || d_out_idx), ALQ_EINVAL, "alq_topk_uncertain: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return topk_impl(ctx, d_keys, n, B, d_out_idx, d_work);
}

size_t alq_topk_mask_work_bytes(int64_t n) { return topk_mask_work_bytes_impl(n); }

int alq_topk_mask(alq_ctx *ctx, const double *d_v, int64_t n, int64_t k, float *d_mask, void *d_work) {
    ALQ_REQUIRE(ctx && (n == 0 || (d_v && d_mask && d_work)), ALQ_EINVAL, "alq_topk_mask: null argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return topk_mask_impl(ctx, d_v, n, k, d_mask, d_work);
}

int alq_threshold_mask(alq_ctx *ctx, const double *d_v, int64_t n, double thr, float *d_mask) {
    ALQ_REQUIRE(ctx && n >= 0 && (n == 0 || (d_v && d_mask)), ALQ_EINVAL, "alq_threshold_mask: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return threshold_mask_impl(ctx, d_v, n, thr, d_mask);
}

int alq_topk_merge(const double *h_keys, const int64_t *h_idx, int64_t n, int64_t B, int64_t *h_out_idx,
                   int64_t *n_out) {
    ALQ_REQUIRE(n >= 0 && B >= 0 && (n == 0 || (h_keys && h_idx)) && (B == 0 || h_out_idx) && n_out, ALQ_EINVAL,
                "alq_topk_merge: bad argument");
    // Keys are compared by BIT PATTERN, like the device top-B (topk.hip): |p - .5| is non-negative, so the unsigned
    // order of the bits is the numeric order, and a NaN key (NaN posterior of a NaN / inf patch on some rank) sorts
    // deterministically behind every number instead of breaking the strict weak ordering of operator<.
    std::vector<std::pair<uint64_t, int64_t>> v;
    v.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i)
        if (h_idx[i] >= 0) {
            double k = h_keys[i] == 0.0 ? 0.0 : h_keys[i];      // -0.0 -> +0.0
            uint64_t b;
            std::memcpy(&b, &k, sizeof(b));
            v.emplace_back(b, h_idx[i]);
        }
    std::sort(v.begin(), v.end());          // key bits, then global index
    const int64_t m = std::min<int64_t>(B, (int64_t)v.size());
    for (int64_t i = 0; i < m; ++i) h_out_idx[i] = v[(size_t)i].second;
    *n_out = m;
    return ALQ_OK;
}

int alq_sgd_step(alq_ctx *ctx, float *d_theta, const float *d_grad, int64_t n, float lr) {
    ALQ_REQUIRE(ctx && (n == 0 || (d_theta && d_grad)) && n >= 0, ALQ_EINVAL, "alq_sgd_step: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return n ? k_sgd(ctx, d_theta, d_grad, n, lr) : ALQ_OK;
}

int alq_adam_step(alq_ctx *ctx, float *d_theta, const float *d_grad, float *d_m, float *d_v, int64_t n, float lr, float beta1,
                  float beta2, float eps, int64_t t) {
    ALQ_REQUIRE(ctx && (n == 0 || (d_theta && d_grad && d_m && d_v)) && n >= 0 && t >= 1, ALQ_EINVAL, "alq_adam_step: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)beta2, (double)t)) / (1.0 - std::pow((double)beta1, (double)t));
    return n ? k_adam(ctx, d_theta, d_grad, d_m, d_v, n, (float)lr_t, beta1, beta2, eps) : ALQ_OK;
}

int alq_rmsprop_step(alq_ctx *ctx, float *d_theta, const float *d_grad, float *d_ms, float *d_mom, int64_t n, float lr, float decay,
                     float momentum, float eps) {
    ALQ_REQUIRE(ctx && (n == 0 || (d_theta && d_grad && d_ms && d_mom)) && n >= 0, ALQ_EINVAL, "alq_rmsprop_step: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return n ? k_rmsprop(ctx, d_theta, d_grad, d_ms, d_mom, n, lr, decay, momentum, eps) : ALQ_OK;
}

int alq_loss_stats(alq_ctx *ctx, const float *d_post, int c, int N, const int32_t *d_labels, const alq_loss_t *loss, double *d_stats3) {
    ALQ_REQUIRE(ctx && d_stats3, ALQ_EINVAL, "alq_loss_stats: null argument");
    ALQ_REQUIRE(N >= 1, ALQ_EINVAL, "alq_loss_stats: N=%d", N);
    ALQ_TRY(loss_check("alq_loss_stats", d_post, c, d_labels, loss));
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_loss_cotangent(ctx, d_post, c, N, d_labels, loss, 1.f, 1.f, nullptr, d_stats3);
}

int alq_sq_accum(alq_ctx *ctx, const float *d_grads, int64_t per_sample_len, int N, double *d_acc) {
    ALQ_REQUIRE(ctx && d_grads && d_acc && per_sample_len >= 1 && N >= 1, ALQ_EINVAL, "alq_sq_accum: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_sq_accum(ctx, d_grads, per_sample_len, N, d_acc);
}

int alq_shrink_sum(alq_ctx *ctx, const float *d_grads, int N, int64_t P, const int64_t *h_layer_elems, int L, double *d_out) {
    ALQ_REQUIRE(ctx && d_grads && h_layer_elems && d_out && N >= 1 && L >= 1 && L <= 64, ALQ_EINVAL, "alq_shrink_sum: bad argument");
    long long off[65];
    off[0] = 0;
    for (int t = 0; t < L; ++t) {
        ALQ_REQUIRE(h_layer_elems[t] >= 1, ALQ_EINVAL, "alq_shrink_sum: layer %d has %lld elements", t, (long long)h_layer_elems[t]);
        off[t + 1] = off[t] + h_layer_elems[t];
    }
    ALQ_REQUIRE(off[L] == P, ALQ_EINVAL, "alq_shrink_sum: the layers hold %lld elements, a gradient row %lld", off[L], (long long)P);
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_shrink_sum(ctx, d_grads, N, P, off, L, d_out);
}

int alq_fisher_classes(alq_ctx *ctx, const double *d_g, const double *d_w, const double *d_diag, int N, int c, int L, double *d_A) {
    ALQ_REQUIRE(ctx && d_g && d_w && d_diag && d_A && N >= 1 && c >= 1 && L >= 1, ALQ_EINVAL, "alq_fisher_classes: bad argument");
    ALQ_HIP(hipSetDevice(ctx->device));
    return k_fisher_classes(ctx, d_g, d_w, d_diag, N, c, L, d_A);
}

int alq_synth_patches(alq_ctx *ctx, uint64_t seed, int64_t first_id, int64_t n, int64_t epp, float *d_out) {
    ALQ_REQUIRE(ctx && (n == 0 || d_out), ALQ_EINVAL, "alq_synth_patches: null argument");
    if (n == 0) return ALQ_OK;
    ALQ_HIP(hipSetDevice(ctx->device));
    return synth_impl(ctx, seed, first_id, n, epp, d_out);
}

}  // extern "C"
