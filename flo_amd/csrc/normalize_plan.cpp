// normalize_plan.cpp — see normalize_plan.hpp.
#include "normalize_plan.hpp"

#include <cmath>

#include "resample_plan.hpp"

namespace flo {

bool normalize_lookahead(uint32_t rate, uint32_t asked, uint32_t &frames, std::string &err) {
    if (asked > kNormMaxLookahead) {
        err = "lookahead_frames " + std::to_string(asked) + " is above the supported " + std::to_string(kNormMaxLookahead);
        return false;
    }
    if (asked) {
        frames = asked;
        return true;
    }
    // round(0.0015 * rate) in integers: (3 * rate + 1000) div 2000
    const uint64_t a = (3ull * rate + 1000) / 2000;
    if (a > kNormMaxLookahead) {
        err = "lookahead_frames: 1.5 ms at " + std::to_string(rate) + " Hz are " + std::to_string(a) + " frames, above the supported " +
              std::to_string(kNormMaxLookahead);
        return false;
    }
    frames = a ? (uint32_t)a : 1u;
    return true;
}

bool normalize_opts(const flo_normalize_opts *in, flo_normalize_opts &out, std::string &err) {
    flo_normalize_opts o;
    o.target_lufs = -14.0;
    o.ceiling_dbtp = -1.0;
    o.max_gain_db = 30.0;
    o.mode = FLO_NORM_GAIN;
    o.lookahead_frames = 0;
    if (in) o = *in;
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    if (!std::isfinite(o.target_lufs)) return bad("target_lufs is not finite");
    if (!std::isfinite(o.ceiling_dbtp) || o.ceiling_dbtp < -60.0 || o.ceiling_dbtp > 60.0) return bad("ceiling_dbtp is outside -60 .. 60");
    if (!(o.max_gain_db >= 0.0 && o.max_gain_db <= 120.0)) return bad("max_gain_db is outside 0 .. 120");
    if (o.mode != FLO_NORM_GAIN && o.mode != FLO_NORM_LIMIT) return bad("mode " + std::to_string(o.mode) + " is neither FLO_NORM_GAIN nor FLO_NORM_LIMIT");
    if (o.lookahead_frames > kNormMaxLookahead)
        return bad("lookahead_frames " + std::to_string(o.lookahead_frames) + " is above the supported " + std::to_string(kNormMaxLookahead));
    out = o;
    return true;
}

float normalize_ceiling(const flo_normalize_opts &o) { return (float)std::pow(10.0, o.ceiling_dbtp / 20.0); }

static double to_db(double linear) { return linear > 1e-9 ? 20.0 * std::log10(linear) : -150.0; }

void normalize_gain(double integrated_lufs, double sample_peak_dbfs, float true_peak, const flo_normalize_opts &o, flo_normalize_report &rep) {
    rep = flo_normalize_report{};
    rep.input_lufs = integrated_lufs;
    rep.input_true_peak = true_peak;
    rep.input_true_peak_dbtp = std::isfinite(true_peak) ? to_db((double)true_peak) : (double)true_peak;
    rep.gain = 1.0f;
    rep.min_gain_q24 = kNormUnity;
    if (!std::isfinite(integrated_lufs) || !std::isfinite(sample_peak_dbfs) || !std::isfinite(true_peak)) {
        rep.status = FLO_NORM_STATUS_NONFINITE;
        return;
    }
    if (sample_peak_dbfs == -150.0) {
        rep.status = FLO_NORM_STATUS_SILENT;
        return;
    }
    double db = o.target_lufs - integrated_lufs;
    if (db > o.max_gain_db) db = o.max_gain_db;
    if (db < -o.max_gain_db) db = -o.max_gain_db;
    float g = (float)std::pow(10.0, db / 20.0);
    const double tp = (double)true_peak;
    const double cap = o.mode == FLO_NORM_GAIN ? (double)normalize_ceiling(o) * kNormGainMargin : kNormMaxScaledPeak;
    bool lowered = false;
    if (tp * (double)g > cap) {
        g = (float)(cap / tp);
        while (tp * (double)g > cap) g = std::nextafterf(g, 0.0f);
        lowered = true;
    }
    rep.gain = g;
    rep.gain_db = 20.0 * std::log10((double)g);
    rep.ceiling_reduction_db = lowered ? db - rep.gain_db : 0.0;
}

std::vector<float> normalize_table() {
    ResamplePlan p;
    std::string err;
    resample_plan(1, kNormPhases, p, err);   // L = 4, M = 1, 64 taps
    return resample_table(p);
}

float normalize_skip_bound(const std::vector<float> &h) {
    double worst = 0;
    for (uint32_t q = 0; q < kNormPhases; q++) {
        double s = 0;
        for (uint32_t k = 0; k < kNormTaps; k++) s += std::fabs((double)h[q * kNormTaps + k]);
        if (s > worst) worst = s;
    }
    const double b = worst * (1.0 + 0x1p-16);
    float f = (float)b;
    if ((double)f < b) f = std::nextafterf(f, INFINITY);
    return f;
}

}  // namespace flo
