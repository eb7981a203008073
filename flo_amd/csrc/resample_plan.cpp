// resample_plan.cpp — see resample_plan.hpp.
#include "resample_plan.hpp"

#include <cmath>
#include <numeric>

namespace flo {

uint32_t resample_span(uint32_t L, uint32_t M, uint32_t taps, uint32_t q) {
    // slot q - 1, phase index L - 1, tap taps - 1 is the last frame read
    const uint64_t s = (uint64_t)(q - 1) * M + (uint64_t)(L - 1) * M / L + taps;
    return s > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)s;
}

static uint64_t plane_bytes(uint32_t L, uint32_t M, uint32_t taps, uint32_t shift, uint32_t q) {
    const uint32_t span = resample_span(L, M, taps, q);
    return ((uint64_t)resample_lds_index(span - 1, shift) + 1) * kResampleFrameBytes;
}

bool resample_plan(uint32_t in_rate, uint32_t out_rate, ResamplePlan &out, std::string &err) {
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    if (in_rate < 1 || in_rate > kResampleMaxRate) return bad("in_rate " + std::to_string(in_rate) + " is outside 1 .. 384000");
    if (out_rate < 1 || out_rate > kResampleMaxRate) return bad("out_rate " + std::to_string(out_rate) + " is outside 1 .. 384000");
    ResamplePlan p;
    p.in_rate = in_rate;
    p.out_rate = out_rate;
    const uint32_t g = std::gcd(in_rate, out_rate);
    p.L = out_rate / g;
    p.M = in_rate / g;
    if (p.L > kResampleMaxPhases)
        return bad("L = out_rate / gcd = " + std::to_string(p.L) + " phases, above the supported " + std::to_string(kResampleMaxPhases));
    // W = 32 / c with c = min(1, L / M); ceil(W) in integers
    const uint64_t half = p.L >= p.M ? 32 : ((uint64_t)32 * p.M + p.L - 1) / p.L;
    if (2 * half > kResampleMaxTaps)
        return bad("taps = " + std::to_string(2 * half) + " per phase, above the supported " + std::to_string(kResampleMaxTaps));
    p.taps = (uint32_t)(2 * half);
    if ((uint64_t)p.L * p.taps * 4 > kResampleMaxTableBytes)
        return bad("table of L * taps * 4 = " + std::to_string((uint64_t)p.L * p.taps * 4) + " bytes, above the supported " +
                   std::to_string(kResampleMaxTableBytes));
    p.cutoff = p.L >= p.M ? 1.0 : (double)p.L / (double)p.M;
    p.W = kResampleZeroCrossings / p.cutoff;
    p.shift = (p.M & 1u) ? 31u : (uint32_t)__builtin_ctz(p.M);
    // the slots of a tile: enough for kResampleTargetUnits wave-units, as many as the LDS budget holds otherwise
    uint32_t q = 64 * ((kResampleTargetUnits + p.L - 1) / p.L);
    if (plane_bytes(p.L, p.M, p.taps, p.shift, q) > kResampleLdsBytes) {
        uint32_t lo = 0, hi = q;   // lo fits (or is 0), hi does not
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (plane_bytes(p.L, p.M, p.taps, p.shift, mid) <= kResampleLdsBytes) lo = mid;
            else hi = mid;
        }
        q = lo;
    }
    if (q == 0) return bad("the input span of one phase, M + taps = " + std::to_string(p.M + p.taps) + " frames, does not fit the LDS of a workgroup");
    if (q > 64) q -= q % 64;
    if (q <= 32) {   // several phases side by side: of the slot counts above q / 2, the one that fills most lanes (the largest such)
        uint32_t best = q;
        for (uint32_t t = q; t > q / 2; t--)
            if ((64 / t) * t > (64 / best) * best) best = t;
        q = best;
    }
    p.slots = q;
    p.tile_outputs = q * p.L;
    p.lanes_per_phase = q < 64 ? q : 64;
    p.phases_per_wave = 64 / p.lanes_per_phase;
    p.chunks = (q + 63) / 64;
    p.block = p.phases_per_wave == 1 ? kResampleBlock : 1;
    p.units = p.chunks * ((p.L + p.phases_per_wave * p.block - 1) / (p.phases_per_wave * p.block));
    p.span = resample_span(p.L, p.M, p.taps, q);
    p.lds_elems = resample_lds_index(p.span - 1, p.shift) + 1;
    out = p;
    return true;
}

// I0 by its power series: every term positive, x <= 9 here (34 terms reach 1e-17 of the sum)
static double bessel_i0(double x) {
    const double q = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

static double sinc_pi(double t) {
    if (t == 0) return 1.0;
    const double y = M_PI * t;
    return std::sin(y) / y;
}

std::vector<float> resample_table(const ResamplePlan &p) {
    const uint32_t L = p.L, T = p.taps;
    std::vector<float> h((size_t)L * T);
    std::vector<double> row(T);
    const double rc = kResampleRho * p.cutoff, i0b = bessel_i0(kResampleBeta);
    for (uint32_t ph = 0; ph < L; ph++) {
        double sum = 0;
        for (uint32_t k = 0; k < T; k++) {
            const double d = ((double)k - (double)(T / 2) + 1.0) - (double)ph / (double)L;
            const double u = d / p.W;
            double v = 0;
            if (std::fabs(u) <= 1.0) v = rc * sinc_pi(rc * d) * bessel_i0(kResampleBeta * std::sqrt(1.0 - u * u)) / i0b;
            row[k] = v;
            sum += v;
        }
        for (uint32_t k = 0; k < T; k++) h[(size_t)ph * T + k] = (float)(row[k] / sum);
    }
    return h;
}

bool resample_out_frames(const ResamplePlan &p, uint64_t n_in, uint64_t &n_out) {
    const unsigned __int128 t = (unsigned __int128)n_in * p.L + (p.M - 1);
    const unsigned __int128 r = t / p.M;
    if (r >> 63) return false;
    n_out = (uint64_t)r;
    return true;
}

uint32_t resample_pass_channels(uint32_t channels) { return channels >= 2 ? 2 : 1; }

uint32_t resample_lds_bytes(const ResamplePlan &p, uint32_t channels) {
    return p.lds_elems * 4 * resample_pass_channels(channels);
}

}  // namespace flo
