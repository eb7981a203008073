// analysis_plan.cpp — see analysis_plan.hpp. Pure host code; built with -ffp-contract=off so every expression rounds step
// by step (the coefficients and M^L are the values the oracle and the kernels' own arithmetic give).
#include "analysis_plan.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

namespace flo {

bool analysis_fast_path(uint64_t frames, unsigned hop, unsigned ch) {
    return frames > 65536 && hop && ch <= 64 && !getenv("FLO_ANALYSIS_EXACT");
}
void analysis_plan(AnalysisPlan &A, size_t n, uint32_t sr, uint8_t ch, uint32_t pps, std::vector<uint64_t> *block_len_out, bool peaks_only,
                   const AnalysisPlan *like) {
    A.n = n;
    A.sample_rate = sr;
    A.channels = ch;
    A.samples_per_peak = (double)sr / (double)pps;
    if (n) {
        const double tp = std::ceil((double)n / (A.samples_per_peak * (double)ch));
        // peak windows that start inside the clip (analysis.rs:54-64: the loop breaks at the first one that does not)
        unsigned np = 0;
        const unsigned cap = tp > 0 ? (tp > 4e9 ? 4000000000u : (unsigned)tp) : 0u;
        while (np < cap && (uint64_t)((double)np * A.samples_per_peak) * ch < n) np++;
        A.n_peaks = np;
    }
    if (!n || peaks_only) return;
    if (like && (!like->n || like->sample_rate != sr)) like = nullptr;
    // K-weighting (ebu_r128.rs:51-103) and block geometry (:190-192, :236-262)
    if (like) {
        memcpy(A.shelf, like->shelf, sizeof A.shelf);
        memcpy(A.hp, like->hp, sizeof A.hp);
        A.hop = like->hop;
    } else {
        const double rate = (double)sr;
        const double f0 = 1681.974450955533, g_db = 3.999843853973347, q = 0.7071752369554196;
        const double k = std::tan(M_PI * f0 / rate), vh = std::pow(10.0, g_db / 20.0), vb = std::pow(vh, 0.4996667741545416);
        const double a0 = 1.0 + k / q + k * k;
        A.shelf[0] = (vh + vb * k / q + k * k) / a0;
        A.shelf[1] = 2.0 * (k * k - vh) / a0;
        A.shelf[2] = (vh - vb * k / q + k * k) / a0;
        A.shelf[3] = 2.0 * (k * k - 1.0) / a0;
        A.shelf[4] = (1.0 - k / q + k * k) / a0;
        const double f0h = 38.13547087602444, qh = 0.5003270373238773, kh = std::tan(M_PI * f0h / rate);
        const double a0h = 1.0 + kh / qh + kh * kh;
        A.hp[0] = 1.0;
        A.hp[1] = -2.0;
        A.hp[2] = 1.0;
        A.hp[3] = 2.0 * (kh * kh - 1.0) / a0h;
        A.hp[4] = (1.0 - kh / qh + kh * kh) / a0h;
        A.hop = (unsigned)std::llround(rate * 0.1);
    }
    const uint64_t frames = n / ch;
    std::vector<uint64_t> block_len;   // (ebu_r128.rs:236-262)
    if (A.hop) {
        uint64_t start = 0;
        const uint64_t block = (uint64_t)A.hop * 4;
        while (start < frames) {
            const uint64_t end = start + block < frames ? start + block : frames;
            if (end <= start) break;
            block_len.push_back(end - start);
            if (end == frames) break;
            start += A.hop;
        }
    }
    A.n_blocks = (unsigned)block_len.size();
    // segments of the order-bound scans (analysis_kernels.hip): a block must not span more than two of them, and the
    // warm-up is a quarter of a second (the 38 Hz high-pass has decayed by exp(-59) then)
    A.seg_frames = 65536u > 8u * A.hop ? 65536u : 8u * A.hop;
    A.warm_frames = 8192u > sr / 4u ? 8192u : sr / 4u;
    {
        const uint64_t longest = (n + ch - 1) / ch;   // samples of channel 0 (a trailing partial frame counts for the FIR)
        A.n_seg = (unsigned)((longest + A.seg_frames - 1) / A.seg_frames);
        if (A.n_seg == 0) A.n_seg = 1;
    }
    A.fast = analysis_fast_path(frames, A.hop, ch) ? 1u : 0u;
    // segment length: two walks of L frames (150 ns per frame) against a scan over frames / L segments (35 ns each):
    // the power of two next to sqrt(frames / 8), between 256 and 2048
    A.kseg_frames = 256;
    while (A.kseg_frames < 2048 && (uint64_t)A.kseg_frames * A.kseg_frames * 8 < frames) A.kseg_frames *= 2;
    A.n_kseg = (unsigned)((frames + A.kseg_frames - 1) / A.kseg_frames);
    A.kq = A.hop ? A.kseg_frames / A.hop + 2 : 1;
    if (A.fast && like && like->fast && like->kseg_frames == A.kseg_frames) {
        memcpy(A.kpow, like->kpow, sizeof A.kpow);
    } else if (A.fast) {
        // M^L: the homogeneous system (x = 0) walked L steps from each unit state, in the kernels' own arithmetic
        for (int col = 0; col < 4; col++) {
            double v[4] = {0, 0, 0, 0};
            v[col] = 1.0;
            for (unsigned i = 0; i < A.kseg_frames; i++) {
                const double y = v[0];
                const double n1 = -A.shelf[3] * y + v[1], n2 = -A.shelf[4] * y;
                const double y2 = A.hp[0] * y + v[2];
                const double m1 = A.hp[1] * y - A.hp[3] * y2 + v[3], m2 = A.hp[2] * y - A.hp[4] * y2;
                v[0] = n1, v[1] = n2, v[2] = m1, v[3] = m2;
            }
            for (int r = 0; r < 4; r++) A.kpow[4 * r + col] = v[r];
        }
    }
    A.sq_seg = 1u << 16;
    A.n_sq_seg = (unsigned)((n + A.sq_seg - 1) / A.sq_seg);
    // beyond one segment the sum of squares is chained chunk by chunk so that it IS the sequential f32 sum (analysis_kernels.hip)
    A.sq_exact = n > A.sq_seg ? 1u : 0u;
    A.n_sq_chunks = (n + 1023) / 1024;
    if (A.sq_exact) A.n_sq_seg = 1;
    if (like) {
        memcpy(A.tp_coef, like->tp_coef, sizeof A.tp_coef);
    } else {   // compute_true_peak's filter (ebu_r128.rs:117-140): 49-tap Hann-windowed sinc, designed at 4 fs, unit sum
        const double oversample_rate = (double)sr * 4.0, cutoff = (double)sr * 0.45, center = 24.0;
        double sum = 0.0;
        for (int i = 0; i < 49; i++) {
            const double nn = (double)i - center;
            const double sinc = std::fabs(nn) < 1e-12 ? 2.0 * cutoff / oversample_rate : std::sin(2.0 * cutoff * nn / oversample_rate) / (M_PI * nn);
            const double window = 0.5 * (1.0 - std::cos(2.0 * M_PI * (double)i / 48.0));
            A.tp_coef[i] = sinc * window;
        }
        for (int i = 0; i < 49; i++) sum += A.tp_coef[i];
        for (int i = 0; i < 49; i++) A.tp_coef[i] /= sum;
    }
    A.n_chunks = (9ull + 4ull * n + 1023ull) / 1024ull;
    const uint64_t spc = n / ch;
    const uint64_t pts[3] = {spc / 4, spc / 2, spc * 3 / 4};
    for (int i = 0; i < 3; i++) {
        A.points[i] = pts[i];
        A.point_ok[i] = pts[i] + 256 < spc ? 1u : 0u;
    }
    if (block_len_out) *block_len_out = std::move(block_len);
}

}  // namespace flo
