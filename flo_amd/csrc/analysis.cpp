// analysis.cpp — analysis metadata (flo_analyze, flo_analysis_metadata, flo_batch_analyze_all and their kin): the host's
// share of the per-clip and of the batched analysis. The kernels live in analysis_kernels.hip / analysis_batch_kernels.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "analysis_plan.hpp"
#include "batch_internal.hpp"
#include "devmem.hpp"

// add_analysis_data_if_missing (lib.rs:219-283) for an empty input META: what libflo::encode / encode_lossy /
// encode_with_bitrate put in front of the encoders. The per-sample work runs on the device (analysis_kernels.hip); what
// is left here is scalar: the K-weighting coefficients (ebu_r128.rs:51-103), the gating of a few hundred block energies
// (:268-318), the u8 scalings of sixteen band energies (analysis.rs:320-341) and the MessagePack framing
// (rmp_serde::to_vec_named of FloMetadata, core/metadata.rs: the fields that are set, in declaration order).
namespace {
struct Mp {
    std::vector<uint8_t> b;
    void u(uint64_t v) {
        if (v < 128) b.push_back((uint8_t)v);
        else if (v < 256) { b.push_back(0xcc); b.push_back((uint8_t)v); }
        else if (v < 65536) { b.push_back(0xcd); b.push_back((uint8_t)(v >> 8)); b.push_back((uint8_t)v); }
        else if (v < 4294967296ull) { b.push_back(0xce); for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(v >> (8 * k))); }
        else { b.push_back(0xcf); for (int k = 7; k >= 0; k--) b.push_back((uint8_t)(v >> (8 * k))); }
    }
    void s(const char *t) {
        const size_t n = strlen(t);
        if (n < 32) b.push_back((uint8_t)(0xa0 | n));
        else { b.push_back(0xd9); b.push_back((uint8_t)n); }
        b.insert(b.end(), t, t + n);
    }
    void f(float x) {
        uint32_t w;
        memcpy(&w, &x, 4);
        b.push_back(0xca);
        for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(w >> (8 * k)));
    }
    void arr(size_t n) {
        if (n < 16) b.push_back((uint8_t)(0x90 | n));
        else if (n < 65536) { b.push_back(0xdc); b.push_back((uint8_t)(n >> 8)); b.push_back((uint8_t)n); }
        else { b.push_back(0xdd); for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(n >> (8 * k))); }
    }
    void bin(const std::vector<uint8_t> &p) {
        const size_t n = p.size();
        if (n < 256) { b.push_back(0xc4); b.push_back((uint8_t)n); }
        else if (n < 65536) { b.push_back(0xc5); b.push_back((uint8_t)(n >> 8)); b.push_back((uint8_t)n); }
        else { b.push_back(0xc6); for (int k = 3; k >= 0; k--) b.push_back((uint8_t)(n >> (8 * k))); }
        b.insert(b.end(), p.begin(), p.end());
    }
};
uint8_t f32_as_u8(float v) {   // Rust `as u8`: saturating, NaN -> 0
    if (!(v == v) || v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}
float max_rust(float a, float b) {
    if (a != a) return b;
    if (b != b) return a;
    return a > b ? a : b;
}
}  // namespace

// a clip's AnalysisArgs but its buffers, from its plan (analysis_plan.cpp); `plan` keeps the plan for a later clip's `like`
static void analysis_geometry(AnalysisArgs &A, size_t n, uint32_t sr, uint8_t ch, uint32_t pps, std::vector<uint64_t> *block_len_out,
                              bool peaks_only = false, const AnalysisPlan *like = nullptr, AnalysisPlan *plan = nullptr) {
    AnalysisPlan P;
    analysis_plan(P, n, sr, ch, pps, block_len_out, peaks_only, like);
    A.n = P.n;
    A.sample_rate = P.sample_rate;
    A.channels = P.channels;
    A.samples_per_peak = P.samples_per_peak;
    A.n_peaks = P.n_peaks;
    memcpy(A.shelf, P.shelf, sizeof A.shelf);
    memcpy(A.hp, P.hp, sizeof A.hp);
    A.hop = P.hop;
    A.n_blocks = P.n_blocks;
    A.seg_frames = P.seg_frames;
    A.warm_frames = P.warm_frames;
    A.n_seg = P.n_seg;
    A.sq_seg = P.sq_seg;
    A.n_sq_seg = P.n_sq_seg;
    A.fast = P.fast;
    A.kseg_frames = P.kseg_frames;
    A.n_kseg = P.n_kseg;
    A.kq = P.kq;
    memcpy(A.kpow, P.kpow, sizeof A.kpow);
    A.sq_exact = P.sq_exact;
    A.n_sq_chunks = P.n_sq_chunks;
    memcpy(A.tp_coef, P.tp_coef, sizeof A.tp_coef);
    A.n_chunks = P.n_chunks;
    for (int i = 0; i < 3; i++) A.points[i] = P.points[i], A.point_ok[i] = P.point_ok[i];
    if (plan) *plan = P;
}
// twiddles of the 256-point FFT: cos / sin in double, rounded to f32 (the values the oracle's FFT uses)
constexpr size_t kAnTwBytes = 8 * 128 * 2 * sizeof(float);
static const float *analysis_twiddles() {
    // (a function-local static initialised by a lambda: thread-safe, contexts on several threads may meet here)
    struct Tw {
        float v[8 * 128 * 2];
    };
    static const Tw tw_table = [] {
        Tw t{};
        for (int s = 0; s < 8; s++)
            for (int k = 0; k < (1 << s); k++) {
                const double ang = -2.0 * M_PI * (double)k / (double)(2 << s);
                t.v[(s * 128 + k) * 2] = (float)std::cos(ang);
                t.v[(s * 128 + k) * 2 + 1] = (float)std::sin(ang);
            }
        return t;
    }();
    return tw_table.v;
}
// what an analysis holds before the device has seen the samples (all of it for an empty clip)
static void analysis_defaults(flo_analysis *out, size_t n, uint32_t sr, uint8_t ch) {
    memset(out, 0, sizeof *out);
    out->sample_rate = sr;
    out->channels = ch;
    out->integrated_lufs = -23.0;
    out->loudness_range_lu = 0.0;
    out->true_peak_dbtp = -150.0;
    out->sample_peak_dbfs = -150.0;
    out->length_ms = (uint64_t)((double)(n / ch) / (double)sr * 1000.0);
}
// what comes back from the device for one clip, and the host's share of the analysis: peak normalisation, the
// fingerprint's u8 scalings, the two gates over the block energies `en` (ebu_r128.rs:268-318) and the peaks in dB
struct AnalysisRaw {
    const float *peaks, *sumsq_part, *band;   // [n_peaks] before normalisation | [n_sq_seg] | [3][16]
    const uint32_t *bin, *root;               // [3][8] | [8]
    const unsigned long long *peak_bits;      // [2]
};
static void analysis_finish(const AnalysisArgs &A, const AnalysisRaw &R, const std::vector<double> &en, float *peaks, flo_analysis *out) {
    const size_t n = A.n;
    const uint32_t sr = A.sample_rate;
    const uint64_t spc = n / A.channels;
    // waveform peaks: normalise by the largest (analysis.rs:103-109)
    {
        const float *pk = R.peaks;
        float mx = 0.f;
        for (unsigned i = 0; i < A.n_peaks; i++) mx = max_rust(mx, pk[i]);
        for (unsigned i = 0; i < A.n_peaks; i++) peaks[i] = mx > 0.f ? pk[i] / mx : pk[i];
    }
    // fingerprint (analysis.rs:236-356)
    {
        const double dms = (double)spc / (double)sr * 1000.0;
        const uint32_t d = dms >= 4294967295.0 ? 4294967295u : (dms <= 0 ? 0u : (uint32_t)dms);
        out->duration_ms = d < 1 ? 1 : d;
        for (int i = 0; i < 8; i++)
            for (int k = 0; k < 4; k++) out->hash[4 * i + k] = (uint8_t)(R.root[i] >> (8 * k));
        const float *bs = R.band;
        const uint32_t *pb = R.bin;
        float bands[16] = {0};
        uint8_t pk8[8] = {0};
        for (int p = 0; p < 3; p++) {
            if (!A.point_ok[p]) continue;
            for (int b = 0; b < 16; b++) bands[b] += bs[p * 16 + b];
            for (int b = 0; b < 8; b++) {
                const uint8_t v = f32_as_u8((float)pb[p * 8 + b] / 256.0f * 255.0f);
                if (v > pk8[b]) pk8[b] = v;
            }
        }
        float mx = 0.f;
        for (int b = 0; b < 16; b++) mx = max_rust(mx, bands[b]);
        for (int b = 0; b < 16; b++) out->energy_profile[b] = mx > 0.f ? f32_as_u8(bands[b] / mx * 255.0f) : 0;
        memcpy(out->frequency_peaks, pk8, 8);
        float sumsq = 0.f;   // the segments' partial sums, in order (one segment: the reference's own sequential sum)
        for (unsigned i = 0; i < A.n_sq_seg; i++) sumsq = i ? sumsq + R.sumsq_part[i] : R.sumsq_part[0];
        out->sum_squares = sumsq;
        if (A.sq_exact && getenv("FLO_TRACE"))
            fprintf(stderr, "[analysis] sum of squares: %llu chunks, %g walked sample by sample\n", (unsigned long long)A.n_sq_chunks,
                    (double)R.sumsq_part[1]);
        const float rms = sumsq / (float)n;
        float v = -20.0f * log10f(rms + 1e-10f);
        if (v == v) v = v < -60.0f ? -60.0f : (v > 0.0f ? 0.0f : v);
        out->avg_loudness = f32_as_u8(v + 60.0f);
    }
    // loudness: the two gates, the range of the gated block loudness and the two peaks (ebu_r128.rs:211-355)
    {
        double lufs = -23.0, lra = 0.0;
        if (!en.empty()) {
            const double abs_gate = std::pow(10.0, (-70.0 + 0.691) / 10.0);
            double sum = 0.0;
            size_t cnt = 0;
            for (double e : en)
                if (e >= abs_gate) {
                    sum += e;
                    cnt++;
                }
            if (cnt) {
                const double ungated = -0.691 + 10.0 * std::log10(sum / (double)cnt);
                const double rel_gate = std::pow(10.0, (ungated - 10.0 + 0.691) / 10.0);
                double s2 = 0.0;
                std::vector<double> vals;
                for (double e : en)
                    if (e >= abs_gate && e >= rel_gate) {
                        s2 += e;
                        vals.push_back(e > 0.0 ? -0.691 + 10.0 * std::log10(e) : -150.0);
                    }
                lufs = !vals.empty() ? -0.691 + 10.0 * std::log10(s2 / (double)vals.size()) : ungated;
                if (vals.size() >= 2) {   // LRA: 10th - 95th percentile, linear interpolation (ebu_r128.rs:320-345)
                    std::sort(vals.begin(), vals.end());
                    const double nn = (double)vals.size();
                    auto interp = [&](double pos) {
                        const size_t i = (size_t)std::floor(pos);
                        const double frac = pos - (double)i;
                        return i + 1 < vals.size() ? vals[i] * (1.0 - frac) + vals[i + 1] * frac : vals[i];
                    };
                    lra = interp(0.95 * (nn - 1.0)) - interp(0.10 * (nn - 1.0));
                }
            }
        }
        out->integrated_lufs = lufs;
        out->loudness_range_lu = lra;
        const unsigned long long *pb = R.peak_bits;
        double sp, tp;
        memcpy(&sp, &pb[0], 8);
        memcpy(&tp, &pb[1], 8);
        out->sample_peak_dbfs = sp > 1e-6 ? 20.0 * std::log10(sp) : -150.0;
        out->true_peak_dbtp = tp > 1e-9 ? 20.0 * std::log10(tp) : -150.0;
    }
}

// ---- buffer layouts: where a clip's results and scratch lie, for the per-clip and for the batched path ----------------
namespace {
constexpr size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }
// the extents both paths' layouts are made of (the kernels index them the same way in either)
struct AnExtents {
    size_t blocks, kq, kstate, sqd, sqr, pkp, cvs;
    explicit AnExtents(const AnalysisArgs &A) {
        const size_t ch = A.channels, tiles = (size_t)(((A.n + ch - 1) / ch + kAnTile - 1) / kAnTile);
        blocks = ch * A.n_blocks * 16;                            // block_part [channels][n_blocks][2]
        kq = A.fast ? ch * A.n_kseg * A.kq * 8 : 0;               // kqpart [channels][n_kseg][kq]
        kstate = A.fast ? ch * A.n_kseg * 32 : 0;                 // kstate [channels][n_kseg][4]
        sqd = A.sq_exact ? (A.n_sq_chunks + 1) * 8 : 0;           // sq_dsum [n_sq_chunks + 1]
        sqr = A.sq_exact ? A.n_sq_chunks * 64 : 0;                // sq_rec [n_sq_chunks][8]
        pkp = A.fast ? tiles * ch * 16 : 0;                       // peak_part [tiles x channels][2]
        cvs = (2 * A.n_chunks + 1) * 32;                          // cvs [2][n_chunks][8], and the root behind them
    }
};
// The per-clip path's result block: peaks | sum of squares [n_sq_seg] | peak bits [2] | block sums | twiddles | band
// [3][16] | bin [3][8] | quanta || filter states (start, refinement end) | chunk records | maxima. Zeroed before the launch and read back behind
// it up to `kst`: what lies behind is fully written by its kernels and stays on the device.
struct AnClipLayout {
    size_t peaks, sumsq, pk, blocks, tw, band, bin, kq, kst, kst2, sqd, sqr, pkp, bytes, cvs_bytes;
    explicit AnClipLayout(const AnalysisArgs &A) {
        const AnExtents E(A);
        peaks = 0;
        sumsq = al16((size_t)A.n_peaks * 4);
        pk = sumsq + al16((size_t)A.n_sq_seg * 4);
        blocks = pk + 16;
        tw = blocks + al16(E.blocks);
        band = tw + kAnTwBytes;
        bin = band + 3 * 16 * 4;
        kq = al16(bin + 3 * 8 * 4);
        kst = kq + E.kq;
        kst2 = kst + E.kstate;
        sqd = kst2 + E.kstate;
        sqr = sqd + E.sqd;
        pkp = sqr + E.sqr;
        bytes = pkp + E.pkp;
        cvs_bytes = E.cvs;
    }
    // the clip's pointers into its result block `rb` and its hash block `cvs`
    void bind(AnalysisArgs &A, char *rb, unsigned int *cvs) const {
        A.peaks = (float *)(rb + peaks);
        A.sumsq_part = (float *)(rb + sumsq);
        A.peak_bits = (unsigned long long *)(rb + pk);
        A.block_part = (double *)(rb + blocks);
        A.fft_tw = (const float *)(rb + tw);
        A.band_sqrt = (float *)(rb + band);
        A.peak_bin = (unsigned int *)(rb + bin);
        A.kqpart = (double *)(rb + kq);
        A.kstate = (double *)(rb + kst);
        A.kstate2 = (double *)(rb + kst2);
        A.sq_dsum = (double *)(rb + sqd);
        A.sq_rec = (double *)(rb + sqr);
        A.peak_part = (double *)(rb + pkp);
        A.cvs = cvs;
    }
};
// the batched path, one clip's results: peaks [n_peaks] | sum of squares [2] | peak bits [2] | band [3][16] | bin [3][8] | root [8] | energies [n_blocks]
struct AnResLayout {
    size_t peaks, sumsq, pk, band, bin, root, en, bytes;
    explicit AnResLayout(const AnalysisArgs &A) {
        peaks = 0;
        sumsq = al16((size_t)A.n_peaks * 4);
        pk = sumsq + 16;
        band = pk + 16;
        bin = band + 3 * 16 * 4;
        root = bin + 3 * 8 * 4;
        en = root + 32;
        bytes = al16(en + (size_t)A.n_blocks * 8);
    }
};
// the batched path, one clip's scratch: zeroed before the group (block sums, quanta) | not (filter states, chunk records, maxima, hash)
struct AnScratch {
    size_t blocks, kq, zbytes, kst, kst2, sqd, sqr, pkp, cvs, ubytes;
    explicit AnScratch(const AnalysisArgs &A) {
        const AnExtents E(A);
        blocks = 0;
        kq = al16(A.fast ? 0 : E.blocks);
        zbytes = al16(kq + E.kq);
        kst = 0;
        kst2 = al16(E.kstate);
        sqd = al16(kst2 + E.kstate);
        sqr = al16(sqd + E.sqd);
        pkp = al16(sqr + E.sqr);
        cvs = al16(pkp + E.pkp);
        ubytes = al16(cvs + (A.n ? E.cvs : 0));
    }
};
}  // namespace

// the analysis' three side streams, made once per context (FLO_ANALYSIS_ONE_STREAM=1: none, everything on the context's stream)
static int analysis_side(flo_ctx *c) {
    if (!c->an_side_ready && !getenv("FLO_ANALYSIS_ONE_STREAM")) {
        HIPCHK(c, hipEventCreateWithFlags(&c->an_side.fork, hipEventDisableTiming));
        for (int i = 0; i < 3; i++) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->an_side.st[i], hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->an_side.join[i], hipEventDisableTiming));
        }
        c->an_side_ready = true;
    }
    return FLO_OK;
}

// pcm_dev: the samples are already on the device (a batch's clip): nothing is staged
static int analyze_impl(flo_ctx *c, const float *pcm, const float *pcm_dev, size_t n, uint32_t sr, uint8_t ch, uint32_t pps, float *peaks,
                        size_t peaks_cap, flo_analysis *out) {
    if (!c || !out || (n && !pcm && !pcm_dev) || !ch || !sr || !pps) return c ? fail(c, FLO_ERR_ARG, "flo_analyze: bad argument") : FLO_ERR_ARG;
    analysis_defaults(out, n, sr, ch);
    HIPCHK(c, hipSetDevice(c->device));
    AnalysisArgs A{};
    std::vector<uint64_t> block_len;
    analysis_geometry(A, n, sr, ch, pps, &block_len);
    out->n_peaks = A.n_peaks;
    if (!n) return FLO_OK;
    if (peaks_cap < A.n_peaks) return fail(c, FLO_ERR_ARG, "flo_analyze: peak buffer too small");
    const uint64_t frames = n / ch;
    const float *tw = analysis_twiddles();
    // device buffers: pcm | results
    DevMem d_pcm, d_res, d_cvs;
    QuiesceOnExit quiesce_d_pcm(c);
    if (!pcm_dev) HIPCHK(c, pool_alloc(&d_pcm.p, n * 4 + 64));
    const AnClipLayout L(A);
    HIPCHK(c, pool_alloc(&d_res.p, L.bytes + 64));
    HIPCHK(c, pool_alloc(&d_cvs.p, L.cvs_bytes + 64));
    int rc = ctx_stager(c);
    if (rc != FLO_OK) return rc;
    if (!pcm_dev) {
        std::vector<UploadSeg> segs{{d_pcm.p, pcm, n * 4}};
        std::string err;
        const auto tu0 = std::chrono::steady_clock::now();
        if (stager_upload(c->stager, segs, c->stream, err) != 0) return fail(c, FLO_ERR_DEVICE, err);
        if (getenv("FLO_TRACE")) {
            hipStreamSynchronize(c->stream);
            fprintf(stderr, "[flo] analysis: upload of %.1f MB took %.0f us (%s)\n", (double)n * 4 / 1e6,
                    (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - tu0).count() / 1e3,
                    stager_upload_choice(c->stager, nullptr, nullptr));
        }
    }
    HIPCHK(c, hipMemsetAsync(d_res.p, 0, L.kst, c->stream));   // (what lies behind is fully written by its kernels)
    HIPCHK(c, hipMemcpyAsync((char *)d_res.p + L.tw, tw, kAnTwBytes, hipMemcpyHostToDevice, c->stream));
    A.pcm = pcm_dev ? pcm_dev : d_pcm.as<float>();
    L.bind(A, (char *)d_res.p, d_cvs.as<unsigned int>());
    if ((rc = analysis_side(c)) != FLO_OK) return rc;
    rc = timed_launch(c, "analysis", [&] { return launch_analysis(A, c->stream, c->an_side_ready ? &c->an_side : nullptr); });
    if (rc != FLO_OK && c->an_side_ready)   // (a failed launch may have left a side stream unjoined: the buffers below must outlive it)
        for (int i = 0; i < 3; i++) hipStreamSynchronize(c->an_side.st[i]);
    if (rc != FLO_OK) {
        hipStreamSynchronize(c->stream);
        return rc;
    }
    std::vector<uint8_t> res(L.kst);   // (what lies behind - filter states, the chunk records of the sum of squares - stays on the device)
    uint32_t root[8];
    HIPCHK(c, hipMemcpyAsync(res.data(), d_res.p, L.kst, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(root, d_cvs.as<unsigned int>() + 2 * A.n_chunks * 8, 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // block energies summed over channels (ebu_r128.rs:211-266)
    std::vector<double> en(A.n_blocks);
    {
        const double *part = (const double *)(res.data() + L.blocks);
        std::vector<double> fastpart;
        if (A.fast) {
            // the segments' shares of every 100 ms quantum, added in segment order; a block is its four quanta, in order
            const uint64_t nq = (frames + A.hop - 1) / A.hop;
            const double *kq = (const double *)(res.data() + L.kq);
            std::vector<double> quanta((size_t)ch * nq, 0.0);
            for (unsigned cc = 0; cc < ch; cc++)
                for (uint64_t sg = 0; sg < A.n_kseg; sg++) {
                    const uint64_t f0 = sg * A.kseg_frames, f1 = std::min<uint64_t>(f0 + A.kseg_frames, frames);
                    if (f1 <= f0) continue;
                    const uint64_t q0 = f0 / A.hop, q1 = (f1 - 1) / A.hop;
                    for (uint64_t q = q0; q <= q1; q++) quanta[(size_t)cc * nq + q] += kq[((size_t)cc * A.n_kseg + sg) * A.kq + (q - q0)];
                }
            fastpart.assign((size_t)ch * A.n_blocks * 2, 0.0);
            for (unsigned cc = 0; cc < ch; cc++)
                for (unsigned k = 0; k < A.n_blocks; k++) {
                    double e = 0.0;
                    for (uint64_t q = k; q < (uint64_t)k + 4 && q < nq; q++) e += quanta[(size_t)cc * nq + q];
                    fastpart[((size_t)cc * A.n_blocks + k) * 2] = e;
                }
            part = fastpart.data();
        }
        std::vector<double> poisoned;
        if (!A.fast && A.n_seg > 1) {
            // Warm-up segments: a later segment restarts its filters from zero a warm-up ahead of its first frame, so a sample
            // that is not finite (or a filter that has overflowed) in an earlier segment - which the sequential recurrence
            // never recovers from: every later output is NaN - is forgotten there. The first segment with a share that is not
            // finite tells: every share a later segment wrote becomes NaN (anb_block_energy_kernel does the same).
            poisoned.assign(part, part + (size_t)ch * A.n_blocks * 2);
            for (unsigned cc = 0; cc < ch; cc++) {
                double *pc = poisoned.data() + (size_t)cc * A.n_blocks * 2;
                uint64_t first = UINT64_MAX;   // the first segment that wrote a share that is not finite
                for (unsigned k = 0; k < A.n_blocks; k++)
                    for (unsigned slot = 0; slot < 2; slot++)
                        if (!std::isfinite(pc[2 * k + slot])) first = std::min<uint64_t>(first, (uint64_t)k * A.hop / A.seg_frames + slot);
                if (first == UINT64_MAX) continue;
                const uint64_t behind = (first + 1) * A.seg_frames;   // the first frame of the segments that forgot
                for (unsigned k = 0; k < A.n_blocks; k++) {
                    const uint64_t start = (uint64_t)k * A.hop, end = start + block_len[k];
                    if (end > behind) pc[2 * k + (start >= behind ? 0 : 1)] = std::numeric_limits<double>::quiet_NaN();
                }
            }
            part = poisoned.data();
        }
        for (unsigned k = 0; k < A.n_blocks; k++) {
            double e = 0.0;
            for (unsigned cc = 0; cc < ch; cc++) {
                const double *pp = part + ((size_t)cc * A.n_blocks + k) * 2;
                e += (pp[0] + pp[1]) / (double)block_len[k];   // (a block inside one segment: x + 0.0, exact)
            }
            en[k] = e;
        }
    }
    AnalysisRaw R{};
    R.peaks = (const float *)(res.data() + L.peaks);
    R.sumsq_part = (const float *)(res.data() + L.sumsq);
    R.band = (const float *)(res.data() + L.band);
    R.bin = (const uint32_t *)(res.data() + L.bin);
    R.root = root;
    R.peak_bits = (const unsigned long long *)(res.data() + L.pk);
    analysis_finish(A, R, en, peaks, out);
    return FLO_OK;
}

extern "C" int flo_analyze(flo_ctx *c, const float *pcm, size_t n, uint32_t sr, uint8_t ch, uint32_t pps, float *peaks,
                           size_t peaks_cap, flo_analysis *out) {
    return analyze_impl(c, pcm, nullptr, n, sr, ch, pps, peaks, peaks_cap, out);
}

// the MessagePack META of one analysis (rmp_serde::to_vec_named of FloMetadata: the fields that are set, in order)
static std::vector<uint8_t> analysis_meta_bytes(const flo_analysis &an, const float *peaks, uint32_t pps, size_t n, uint32_t sr, uint8_t ch) {
    Mp m, fp;
    m.b.push_back(0x84);
    m.s("length_ms");
    m.u(an.length_ms);
    m.s("waveform_data");
    m.b.push_back(0x83);
    m.s("peaks_per_second");
    m.u(pps);
    m.s("peaks");
    m.arr(an.n_peaks);
    for (unsigned i = 0; i < an.n_peaks; i++) m.f(peaks[i]);
    m.s("channels");
    m.u(ch);
    m.s("spectrum_fingerprint");
    fp.b.push_back(0x87);
    fp.s("hash");
    fp.arr(32);
    for (int i = 0; i < 32; i++) fp.u(n ? an.hash[i] : 0);
    fp.s("duration_ms");
    fp.u(n ? an.duration_ms : 0);
    fp.s("sample_rate");
    fp.u(sr);
    fp.s("channels");
    fp.u(ch);
    fp.s("frequency_peaks");
    fp.arr(8);
    for (int i = 0; i < 8; i++) fp.u(an.frequency_peaks[i]);
    fp.s("energy_profile");
    fp.arr(16);
    for (int i = 0; i < 16; i++) fp.u(an.energy_profile[i]);
    fp.s("avg_loudness");
    fp.u(an.avg_loudness);
    m.bin(fp.b);
    m.s("loudness_profile");
    m.b.push_back(0x91);
    m.b.push_back(0x82);
    m.s("timestamp_ms");
    m.u(0);
    m.s("lufs");
    m.f((float)an.integrated_lufs);
    return std::move(m.b);
}
static int analysis_metadata_impl(flo_ctx *c, const float *pcm, const float *pcm_dev, size_t n, uint32_t sr, uint8_t ch, uint32_t pps,
                                  uint8_t **out, size_t *out_len) {
    if (!c || !out || !out_len) return FLO_ERR_ARG;
    *out = nullptr;
    *out_len = 0;
    if (!ch || !sr || !pps) return fail(c, FLO_ERR_ARG, "flo_analysis_metadata: bad argument");
    // (one peak per 1 / pps seconds: ceil(frames * pps / rate) of them - a vector of one float per sample frame was 32 MB of
    // zeroed fresh pages for a 3-minute clip, 4 ms of a 7 ms call)
    std::vector<float> peaks((size_t)std::ceil((double)(n / ch) * (double)pps / (double)sr) + 16);
    flo_analysis an;
    int rc = analyze_impl(c, pcm, pcm_dev, n, sr, ch, pps, peaks.data(), peaks.size(), &an);
    if (rc != FLO_OK) return rc;
    const std::vector<uint8_t> mb = analysis_meta_bytes(an, peaks.data(), pps, n, sr, ch);
    uint8_t *p = (uint8_t *)malloc(mb.size());
    if (!p) return fail(c, FLO_ERR_NOMEM, "malloc failed");
    memcpy(p, mb.data(), mb.size());
    *out = p;
    *out_len = mb.size();
    return FLO_OK;
}
extern "C" int flo_analysis_metadata(flo_ctx *c, const float *pcm, size_t n, uint32_t sr, uint8_t ch, uint32_t pps,
                                     uint8_t **out, size_t *out_len) {
    return analysis_metadata_impl(c, pcm, nullptr, n, sr, ch, pps, out, out_len);
}
// the same from a clip that is already on the device (uploaded into a batch that is about to be encoded): libflo::encode*
// analyse and encode the same samples (lib.rs:105-116), and they cross PCIe once
extern "C" int flo_batch_analysis_metadata(flo_batch *b, size_t clip, uint32_t pps, uint8_t **out, size_t *out_len) {
    if (!b || clip >= b->n_clips) return FLO_ERR_ARG;
    return analysis_metadata_impl(b->ctx, nullptr, b->n_il[clip] ? b->d_pcm + b->clip_off[clip] : nullptr, b->n_il[clip], b->sr, b->ch, pps, out, out_len);
}
// ------------------------------------------------------------------------------------------------ batched analysis
// flo_batch_analyze_all: every clip's AnalysisArgs (the per-clip geometry, analysis_geometry) becomes a descriptor, the
// kernels of launch_analysis_batch (analysis_batch_kernels.hip) run over groups of clips - one fixed set of launches per
// group - and one read-back brings every clip's results home: the raw peaks, the fingerprint's pieces, the two peak maxima
// and the block energies, already built on the device in the host's order of additions. The host's share per clip is that
// of the per-clip path (analysis_finish). A group's scratch (filter states, quanta, the chunk records of the sum of
// squares, the hash's chaining values; ~460 KB for 10 s of stereo) stays under FLO_BATCH_ANALYSIS_GROUP_BYTES (1 GiB).
namespace {
struct AnGroup {
    size_t first = 0, count = 0, zbytes = 0, ubytes = 0, pre_off = 0;
    unsigned long long total[kAnlCount] = {};
};
}  // namespace

// workgroups of every list for one clip (an_batch_per_wg items each)
static void an_batch_wgs(const AnalysisArgs &A, unsigned long long (&wg)[kAnlCount]) {
    an_batch_items(A, wg);
    for (int k = 0; k < kAnlCount; k++) wg[k] = (wg[k] + an_batch_per_wg(k) - 1) / an_batch_per_wg(k);
}
static size_t batch_analysis_group_bytes() {
    const char *e = getenv("FLO_BATCH_ANALYSIS_GROUP_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)1 << 30);
}

static void batch_peak_offsets(const flo_batch *b, uint32_t pps, std::vector<AnalysisArgs> &A, uint64_t *peak_off) {
    A.assign(b->n_clips, AnalysisArgs{});
    peak_off[0] = 0;
    for (size_t i = 0; i < b->n_clips; i++) {
        analysis_geometry(A[i], b->n_il[i], b->sr, b->ch, pps, nullptr, true);
        peak_off[i + 1] = peak_off[i] + A[i].n_peaks;
    }
}

extern "C" int flo_batch_analyze_all(flo_batch *b, uint32_t pps, flo_analysis *out, float *peaks, size_t peaks_cap, uint64_t *peak_off) {
    if (!b) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (!pps) return fail(c, FLO_ERR_ARG, "flo_batch_analyze_all: peaks_per_second must be non-zero");
    if (!peak_off || (peaks && !out)) return fail(c, FLO_ERR_ARG, "flo_batch_analyze_all: NULL output");
    std::vector<AnalysisArgs> A;
    batch_peak_offsets(b, pps, A, peak_off);
    if (!peaks) return FLO_OK;   // the sizing call
    const size_t n_clips = b->n_clips;
    if (peaks_cap < peak_off[n_clips]) return fail(c, FLO_ERR_ARG, "flo_batch_analyze_all: peak buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    for (size_t i = 0; i < n_clips; i++) {
        analysis_defaults(&out[i], b->n_il[i], b->sr, b->ch);
        out[i].n_peaks = A[i].n_peaks;
    }
    if (!n_clips) return FLO_OK;
    // geometry, results and scratch of every clip; the groups
    std::vector<size_t> res_off(n_clips + 1, 0), z_off(n_clips), u_off(n_clips), stage_off(n_clips, SIZE_MAX);
    std::vector<AnGroup> groups;
    const size_t cap = batch_analysis_group_bytes();
    const unsigned long long max_items = 1ull << 22;   // workgroups per launch (a single clip may have more, as alone)
    size_t stage_floats = 0;
    AnalysisPlan plan, like_plan;
    const AnalysisPlan *like = nullptr;   // (the last clip with samples: its rate's coefficients are reused)
    for (size_t i = 0; i < n_clips; i++) {
        A[i] = AnalysisArgs{};
        analysis_geometry(A[i], b->n_il[i], b->sr, b->ch, pps, nullptr, false, like, &plan);
        if (A[i].n) like_plan = plan, like = &like_plan;
        res_off[i + 1] = res_off[i] + AnResLayout(A[i]).bytes;
        if (i < b->tail.size() && !b->tail[i].empty()) {   // an odd-length lossy clip: staged whole (frames, then the tail)
            stage_off[i] = stage_floats;
            stage_floats += al16(b->n_il[i] * 4 + 64) / 4;
        }
        const AnScratch S(A[i]);
        unsigned long long it[kAnlCount];
        an_batch_wgs(A[i], it);
        bool fits = !groups.empty() && groups.back().zbytes + groups.back().ubytes + S.zbytes + S.ubytes <= cap;
        for (int k = 0; fits && k < kAnlCount; k++) fits = groups.back().total[k] + it[k] <= max_items;
        if (!fits) {
            groups.emplace_back();
            groups.back().first = i;
        }
        AnGroup &g = groups.back();
        z_off[i] = g.zbytes;
        u_off[i] = g.ubytes;
        g.zbytes += S.zbytes;
        g.ubytes += S.ubytes;
        g.count++;
        for (int k = 0; k < kAnlCount; k++) g.total[k] += it[k];
    }
    size_t scratch_bytes = 16;
    for (const AnGroup &g : groups) scratch_bytes = std::max(scratch_bytes, al16(g.zbytes) + g.ubytes);
    // one upload: descriptors | twiddles | the work lists' prefixes of every group
    const size_t o_tw = al16(n_clips * sizeof(AnalysisArgs)), o_pre = o_tw + kAnTwBytes;
    size_t pre_words = 0;
    for (AnGroup &g : groups) {
        g.pre_off = pre_words;
        pre_words += (size_t)kAnlCount * (g.count + 1);
    }
    std::vector<uint8_t> up(o_pre + pre_words * 4, 0);   // (outlives the stream: destroyed behind `quiesce`)
    DevMem d_desc, d_res, d_scr, d_stage;
    QuiesceOnExit quiesce(c);
    HIPCHK(c, pool_alloc(&d_desc.p, o_pre + pre_words * 4 + 64));
    HIPCHK(c, pool_alloc(&d_res.p, res_off[n_clips] + 64));
    HIPCHK(c, pool_alloc(&d_scr.p, scratch_bytes + 64));
    if (stage_floats) HIPCHK(c, pool_alloc(&d_stage.p, stage_floats * 4 + 64));
    char *rb = (char *)d_res.p, *sb = (char *)d_scr.p;
    const float *d_tw = (const float *)((char *)d_desc.p + o_tw);
    for (const AnGroup &g : groups) {
        uint32_t *pre = (uint32_t *)(up.data() + o_pre) + g.pre_off;
        for (int k = 0; k < kAnlCount; k++) pre[(size_t)k * (g.count + 1)] = 0;
        for (size_t j = 0; j < g.count; j++) {
            const size_t i = g.first + j;
            AnalysisArgs &a = A[i];
            unsigned long long it[kAnlCount];
            an_batch_wgs(a, it);
            for (int k = 0; k < kAnlCount; k++) pre[(size_t)k * (g.count + 1) + j + 1] = pre[(size_t)k * (g.count + 1) + j] + (uint32_t)it[k];
            a.pcm = stage_off[i] != SIZE_MAX ? d_stage.as<float>() + stage_off[i] : b->d_pcm + b->clip_off[i];
            const AnResLayout R(a);
            char *r = rb + res_off[i];
            a.peaks = (float *)(r + R.peaks);
            a.sumsq_part = (float *)(r + R.sumsq);
            a.peak_bits = (unsigned long long *)(r + R.pk);
            a.band_sqrt = (float *)(r + R.band);
            a.peak_bin = (unsigned int *)(r + R.bin);
            a.root = (unsigned int *)(r + R.root);
            a.block_energy = (double *)(r + R.en);
            a.fft_tw = d_tw;
            const AnScratch S(a);
            char *z = sb + z_off[i], *u = sb + al16(g.zbytes) + u_off[i];
            a.block_part = (double *)(z + S.blocks);
            a.kqpart = (double *)(z + S.kq);
            a.kstate = (double *)(u + S.kst);
            a.kstate2 = (double *)(u + S.kst2);
            a.sq_dsum = (double *)(u + S.sqd);
            a.sq_rec = (double *)(u + S.sqr);
            a.peak_part = (double *)(u + S.pkp);
            a.cvs = (unsigned int *)(u + S.cvs);
        }
    }
    memcpy(up.data(), A.data(), n_clips * sizeof(AnalysisArgs));
    memcpy(up.data() + o_tw, analysis_twiddles(), kAnTwBytes);
    HIPCHK(c, hipMemcpyAsync(d_desc.p, up.data(), up.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_res.p, 0, res_off[n_clips], c->stream));
    for (size_t i = 0; i < n_clips; i++)
        if (stage_off[i] != SIZE_MAX) {
            float *dst = d_stage.as<float>() + stage_off[i];
            const size_t whole = b->clip_nsf[i] * b->ch, nt = b->tail[i].size();
            if (whole) HIPCHK(c, hipMemcpyAsync(dst, b->d_pcm + b->clip_off[i], whole * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(dst + whole, b->tail[i].data(), nt * 4, hipMemcpyHostToDevice, c->stream));
        }
    int rc = analysis_side(c);
    if (rc != FLO_OK) return rc;
    const AnalysisArgs *d_clips = (const AnalysisArgs *)d_desc.p;
    const uint32_t *d_pre = (const uint32_t *)((char *)d_desc.p + o_pre);
    for (const AnGroup &g : groups) {
        if (g.zbytes) HIPCHK(c, hipMemsetAsync(sb, 0, g.zbytes, c->stream));   // (the previous group's kernels on this stream are done with it)
        const AnBatchArgs G{d_clips + g.first, d_pre + g.pre_off, (unsigned)g.count};
        rc = timed_launch(c, "analysis_batch", [&] { return launch_analysis_batch(G, g.total, c->stream, c->an_side_ready ? &c->an_side : nullptr); });
        if (rc != FLO_OK) {
            if (c->an_side_ready)   // (a failed launch may have left a side stream unjoined: the buffers must outlive it)
                for (int i = 0; i < 3; i++) hipStreamSynchronize(c->an_side.st[i]);
            hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    std::vector<uint8_t> res(res_off[n_clips]);
    HIPCHK(c, hipMemcpyAsync(res.data(), d_res.p, res.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n_clips; i++) {
        if (!A[i].n) continue;
        const AnResLayout L(A[i]);
        const uint8_t *r = res.data() + res_off[i];
        AnalysisRaw R{};
        R.peaks = (const float *)(r + L.peaks);
        R.sumsq_part = (const float *)(r + L.sumsq);
        R.band = (const float *)(r + L.band);
        R.bin = (const uint32_t *)(r + L.bin);
        R.root = (const uint32_t *)(r + L.root);
        R.peak_bits = (const unsigned long long *)(r + L.pk);
        const double *e = (const double *)(r + L.en);
        analysis_finish(A[i], R, std::vector<double>(e, e + A[i].n_blocks), peaks + peak_off[i], &out[i]);
    }
    return FLO_OK;
}

extern "C" int flo_batch_analysis_metadata_all(flo_batch *b, uint32_t pps, uint8_t **out, uint64_t *off) {
    if (!b) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (!out || !off) return fail(c, FLO_ERR_ARG, "flo_batch_analysis_metadata_all: NULL output");
    *out = nullptr;
    std::vector<uint64_t> poff(b->n_clips + 1);
    int rc = flo_batch_analyze_all(b, pps, nullptr, nullptr, 0, poff.data());
    if (rc != FLO_OK) return rc;
    std::vector<float> peaks(poff[b->n_clips] + 1);
    std::vector<flo_analysis> an(b->n_clips);
    if ((rc = flo_batch_analyze_all(b, pps, an.data(), peaks.data(), peaks.size(), poff.data())) != FLO_OK) return rc;
    std::vector<uint8_t> all;
    off[0] = 0;
    for (size_t i = 0; i < b->n_clips; i++) {
        const std::vector<uint8_t> m = analysis_meta_bytes(an[i], peaks.data() + poff[i], pps, b->n_il[i], b->sr, b->ch);
        all.insert(all.end(), m.begin(), m.end());
        off[i + 1] = all.size();
    }
    uint8_t *p = (uint8_t *)malloc(all.size() ? all.size() : 1);
    if (!p) return fail(c, FLO_ERR_NOMEM, "malloc failed");
    if (!all.empty()) memcpy(p, all.data(), all.size());
    *out = p;
    return FLO_OK;
}
