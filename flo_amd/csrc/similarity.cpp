// similarity.cpp — flo_spectral_similarity and flo_fpindex_*: spectral_similarity (core/analysis.rs:395-437) for one pair
// on the host, and for whole fingerprint sets on the device (similarity_kernels.hip).
//
// flo_fpindex_create turns each fingerprint into its 32-byte device record once: the profile bytes, the loudness, a
// format id per distinct (sample_rate, channels) and a hash id per distinct 32-byte hash (ids in the hashes' sorted
// order, so that a query's hash is found by binary search). Queries are turned into records against the same ids; a hash
// or a format no member has gets an id no member has. Per call: the records of the queries, the chunked pair kernels, the
// merges, one copy back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "devmem.hpp"
#include "similarity_kernels.hpp"

namespace flo {
void fp_term_table(float *t) {
    for (int d = 0; d < 256; d++) t[d] = 1.0f - (float)d / 255.0f;   // contraction off (Makefile): two roundings
}
}  // namespace flo

namespace {

using Hash = std::array<uint8_t, 32>;

const float *term_table() {
    static const std::array<float, 256> t = [] {
        std::array<float, 256> x{};
        fp_term_table(x.data());
        return x;
    }();
    return t.data();
}

// the profile bytes of a fingerprint into record words (w[0..6]; the ids are set by the caller)
void pack_profile(const flo_fingerprint &f, uint32_t *w) {
    for (int k = 0; k < 4; k++)
        w[k] = (uint32_t)f.energy_profile[4 * k] | (uint32_t)f.energy_profile[4 * k + 1] << 8 |
               (uint32_t)f.energy_profile[4 * k + 2] << 16 | (uint32_t)f.energy_profile[4 * k + 3] << 24;
    for (int k = 0; k < 2; k++)
        w[4 + k] = (uint32_t)f.frequency_peaks[4 * k] | (uint32_t)f.frequency_peaks[4 * k + 1] << 8 |
                   (uint32_t)f.frequency_peaks[4 * k + 2] << 16 | (uint32_t)f.frequency_peaks[4 * k + 3] << 24;
    w[6] = f.avg_loudness;
}

uint64_t fmt_key(const flo_fingerprint &f) { return (uint64_t)f.sample_rate << 8 | f.channels; }

}  // namespace

struct flo_fpindex {
    flo_ctx *ctx = nullptr;
    uint32_t n = 0;
    std::vector<Hash> hashes;                 // distinct member hashes, sorted: hash id = position
    std::map<uint64_t, uint32_t> formats;     // (sample_rate, channels) -> format id
    FpRec *d_rec = nullptr;                   // [n]
    float *d_table = nullptr;                 // [256]
};

extern "C" float flo_spectral_similarity(const flo_fingerprint *a, const flo_fingerprint *b) {
    if (!a || !b) return 0.0f;
    if (std::memcmp(a->hash, b->hash, 32) == 0) return 1.0f;
    if (a->sample_rate != b->sample_rate || a->channels != b->channels) return 0.0f;
    uint32_t wa[8], wb[8];
    pack_profile(*a, wa);
    pack_profile(*b, wb);
    return fp_chain_score(wa, wb, term_table());
}

extern "C" void flo_fpindex_destroy(flo_fpindex *ix) {
    if (!ix) return;
    if (ix->ctx && ix->ctx->stream) hipStreamSynchronize(ix->ctx->stream);
    if (ix->d_rec) pool_free(ix->d_rec);
    if (ix->d_table) pool_free(ix->d_table);
    delete ix;
}

// the record of fingerprint f against the index's ids
static FpRec make_rec(const flo_fpindex *ix, const flo_fingerprint &f) {
    FpRec r{};
    pack_profile(f, r.w);
    auto fm = ix->formats.find(fmt_key(f));
    r.w[6] |= (fm == ix->formats.end() ? kFpFmtNone : fm->second) << 8;
    Hash h;
    std::memcpy(h.data(), f.hash, 32);
    auto it = std::lower_bound(ix->hashes.begin(), ix->hashes.end(), h);
    r.w[7] = (it != ix->hashes.end() && *it == h) ? (uint32_t)(it - ix->hashes.begin()) : kFpHashNone;
    return r;
}

extern "C" int flo_fpindex_create(flo_ctx *ctx, const flo_fingerprint *fps, size_t n, flo_fpindex **out) {
    if (!ctx || !out || (n && !fps)) return fail(ctx, FLO_ERR_ARG, "null argument");
    *out = nullptr;
    if (n >= 0xFFFFFFFFu) return fail(ctx, FLO_ERR_ARG, "an index holds fewer than 2^32 - 1 fingerprints");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    flo_fpindex *ix = new flo_fpindex();
    ix->ctx = ctx;
    ix->n = (uint32_t)n;
    auto bail = [&](int rc) {
        flo_fpindex_destroy(ix);
        return rc;
    };
    ix->hashes.resize(n);
    for (size_t i = 0; i < n; i++) {
        std::memcpy(ix->hashes[i].data(), fps[i].hash, 32);
        ix->formats.emplace(fmt_key(fps[i]), 0u);
    }
    std::sort(ix->hashes.begin(), ix->hashes.end());
    ix->hashes.erase(std::unique(ix->hashes.begin(), ix->hashes.end()), ix->hashes.end());
    if (ix->formats.size() >= kFpFmtNone) return bail(fail(ctx, FLO_ERR_ARG, "too many distinct formats"));
    uint32_t id = 0;
    for (auto &f : ix->formats) f.second = id++;
    std::vector<FpRec> rec(n);
    for (size_t i = 0; i < n; i++) rec[i] = make_rec(ix, fps[i]);
    if (pool_alloc(&ix->d_rec, (n ? n : 1) * sizeof(FpRec)) != hipSuccess || pool_alloc(&ix->d_table, 256 * sizeof(float)) != hipSuccess)
        return bail(fail(ctx, FLO_ERR_NOMEM, "fingerprint index"));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ix->d_rec, rec.data(), n * sizeof(FpRec), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ix->d_table, term_table(), 256 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(fail(ctx, FLO_ERR_DEVICE, "fingerprint index upload failed"));
    *out = ix;
    return FLO_OK;
}

// References per chunk: enough chunks that the (query tile x chunk) grid covers the device about four times over, chunks of
// whole LDS tiles, the per-chunk lists of a top-k call within 1 GiB. FLO_FPINDEX_CHUNK_REFS (read per call) forces a
// chunk length instead (tests: results must not depend on it).
static uint32_t choose_chunk(const flo_fpindex *ix, uint32_t n_q, uint32_t n_ref, uint32_t q_lanes, uint64_t list_bytes_per_chunk) {
    uint64_t chunk;
    if (const char *e = std::getenv("FLO_FPINDEX_CHUNK_REFS"); e && std::strtoull(e, nullptr, 10) > 0) {
        chunk = std::strtoull(e, nullptr, 10);
    } else {
        const uint64_t tiles = ((uint64_t)n_q + q_lanes - 1) / q_lanes;
        const uint64_t want = std::max<uint64_t>(1, (4ull * std::max(ix->ctx->prop.multiProcessorCount, 1) + tiles - 1) / tiles);
        chunk = ((uint64_t)n_ref + want - 1) / want;
    }
    chunk = std::max<uint64_t>(kFpTile, (chunk + kFpTile - 1) / kFpTile * kFpTile);
    while (list_bytes_per_chunk && chunk < n_ref && ((uint64_t)n_ref + chunk - 1) / chunk * list_bytes_per_chunk > (1ull << 30))
        chunk *= 2;
    return (uint32_t)std::min<uint64_t>(chunk, 0x80000000ull);
}

static int topk_run(flo_fpindex *ix, const FpRec *d_q, uint32_t n_q, uint32_t k, bool self, uint32_t *idx, float *score) {
    flo_ctx *ctx = ix->ctx;
    const size_t n_out = (size_t)n_q * k;
    if (ix->n == 0) {   // nothing to list: every slot is padding
        std::fill(idx, idx + n_out, 0xFFFFFFFFu);
        std::fill(score, score + n_out, -1.0f);
        return FLO_OK;
    }
    const uint64_t list_bytes = (uint64_t)n_out * 8;
    const uint32_t chunk = choose_chunk(ix, n_q, ix->n, k <= 16 ? kFpTile : 64, list_bytes);
    const uint32_t nc = (ix->n + chunk - 1) / chunk;
    DevBuf<uint32_t> oi, pi, si;
    DevBuf<float> os, ps, ss;
    QuiesceOnExit quiesce(ctx);
    if (!oi.alloc(n_out) || !os.alloc(n_out)) return fail(ctx, FLO_ERR_NOMEM, "top-k results");
    if (nc > 1 && (!pi.alloc(n_out * nc) || !ps.alloc(n_out * nc) || !si.alloc(n_out * ((nc + 1) / 2)) ||
                   !ss.alloc(n_out * ((nc + 1) / 2))))
        return fail(ctx, FLO_ERR_NOMEM, "top-k chunk lists");
    FpTopkArgs a{};
    a.q = d_q;
    a.ref = ix->d_rec;
    a.table = ix->d_table;
    a.n_q = n_q;
    a.n_ref = ix->n;
    a.chunk = chunk;
    a.k = k;
    a.self = self ? 1u : 0u;
    a.part_idx = pi.p;
    a.part_score = ps.p;
    int rc = timed_launch(ctx, "fp_topk", [&] { return launch_fp_topk(a, oi.p, os.p, si.p, ss.p, ctx->stream); });
    if (rc != FLO_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(idx, oi.p, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(score, os.p, n_out * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FLO_OK;
}

extern "C" int flo_fpindex_topk(flo_fpindex *ix, const flo_fingerprint *q, size_t n_q, uint32_t k, uint32_t *idx, float *score) {
    if (!ix) return FLO_ERR_ARG;
    flo_ctx *ctx = ix->ctx;
    if (k > kFpMaxK) return fail(ctx, FLO_ERR_ARG, "k must be at most " + std::to_string(kFpMaxK));
    if (!n_q || !k) return FLO_OK;
    if (!q || !idx || !score) return fail(ctx, FLO_ERR_ARG, "null argument");
    if (n_q >= 0x80000000ull) return fail(ctx, FLO_ERR_ARG, "too many queries in one call");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<FpRec> rec(n_q);
    for (size_t i = 0; i < n_q; i++) rec[i] = make_rec(ix, q[i]);
    DevBuf<FpRec> dq;
    QuiesceOnExit quiesce(ctx);
    if (!dq.alloc(n_q)) return fail(ctx, FLO_ERR_NOMEM, "queries");
    HIPCHK(ctx, hipMemcpyAsync(dq.p, rec.data(), n_q * sizeof(FpRec), hipMemcpyHostToDevice, ctx->stream));
    return topk_run(ix, dq.p, (uint32_t)n_q, k, false, idx, score);
}

extern "C" int flo_fpindex_topk_self(flo_fpindex *ix, uint32_t k, uint32_t *idx, float *score) {
    if (!ix) return FLO_ERR_ARG;
    flo_ctx *ctx = ix->ctx;
    if (k > kFpMaxK) return fail(ctx, FLO_ERR_ARG, "k must be at most " + std::to_string(kFpMaxK));
    if (!ix->n || !k) return FLO_OK;
    if (!idx || !score) return fail(ctx, FLO_ERR_ARG, "null argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return topk_run(ix, ix->d_rec, ix->n, k, true, idx, score);
}

extern "C" int flo_fpindex_pairs(flo_fpindex *ix, float threshold, uint64_t cap, uint32_t *i, uint32_t *j, float *score,
                                 uint64_t *n_pairs) {
    if (!ix) return FLO_ERR_ARG;
    flo_ctx *ctx = ix->ctx;
    if (!n_pairs) return fail(ctx, FLO_ERR_ARG, "null argument");
    *n_pairs = 0;
    if (std::isnan(threshold)) return fail(ctx, FLO_ERR_ARG, "threshold is NaN");
    const uint32_t n = ix->n;
    if (n < 2) return FLO_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint32_t chunk = choose_chunk(ix, n, n, kFpTile, 0);
    const uint32_t nc = (n + chunk - 1) / chunk;
    const size_t cells = (size_t)n * nc;
    DevBuf<uint32_t> dcount, di, dj;
    DevBuf<unsigned long long> doff;
    DevBuf<float> ds;
    QuiesceOnExit quiesce(ctx);
    if (!dcount.alloc(cells)) return fail(ctx, FLO_ERR_NOMEM, "pair counts");
    FpPairsArgs a{};
    a.rec = ix->d_rec;
    a.table = ix->d_table;
    a.n = n;
    a.chunk = chunk;
    a.threshold = threshold;
    a.count = dcount.p;
    int rc = timed_launch(ctx, "fp_pairs_count", [&] { return launch_fp_pairs_count(a, ctx->stream); });
    if (rc != FLO_OK) return rc;
    std::vector<uint32_t> count(cells);
    HIPCHK(ctx, hipMemcpyAsync(count.data(), dcount.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> off(cells);
    uint64_t total = 0;
    for (size_t c = 0; c < cells; c++) {
        off[c] = total;
        total += count[c];
    }
    *n_pairs = total;
    if (total > cap)
        return fail(ctx, FLO_ERR_NOMEM, std::to_string(total) + " pairs at or above the threshold, room for " + std::to_string(cap));
    if (!total) return FLO_OK;
    if (!i || !j || !score) return fail(ctx, FLO_ERR_ARG, "null argument");
    if (!doff.alloc(cells) || !di.alloc(total) || !dj.alloc(total) || !ds.alloc(total))
        return fail(ctx, FLO_ERR_NOMEM, "pair output");
    HIPCHK(ctx, hipMemcpyAsync(doff.p, off.data(), cells * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    a.count = nullptr;
    a.off = doff.p;
    a.cap = total;
    a.pi = di.p;
    a.pj = dj.p;
    a.ps = ds.p;
    rc = timed_launch(ctx, "fp_pairs_write", [&] { return launch_fp_pairs_write(a, ctx->stream); });
    if (rc != FLO_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(i, di.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(j, dj.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(score, ds.p, total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return FLO_OK;
}
