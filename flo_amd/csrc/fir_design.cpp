// fir_design.cpp — flo_fir_design: windowed-sinc FIR tables for flo_batch_convolve (Kaiser window, all arithmetic in f64,
// rounded to f32 once at the end). Plain C++, no device: a host test builds it with g++ alone
// (tests/native/conv_plan_test.cpp). The definition is include/flo_hip.h's and DESIGN 4.18's.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "conv_plan.hpp"

namespace flo {

// I0 by its power series and sinc: restated from resample_plan.cpp, whose table is pinned by its tests, operation for
// operation. Every term is positive. The terms grow up to k = x / 2 and fall from there; counted with this loop, it ends
// after 32 terms at x = 16 (the largest beta) and after 24 at x = 9, far from the cap of 200.
static double fir_bessel_i0(double x) {
    const double q = x * x / 4;
    double term = 1, sum = 1;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

static double fir_sinc_pi(double t) {
    if (t == 0) return 1.0;
    const double y = M_PI * t;
    return std::sin(y) / y;
}

// lp(f)[k] = g[k] / sum(g), g[k] = (2f/R) sinc(2f (k - H)/R) I0(beta sqrt(1 - ((k - H)/H)^2)) / I0(beta)
static std::vector<double> fir_lowpass(double f, double rate, uint32_t taps, double beta) {
    const uint32_t H = taps / 2;
    const double i0b = fir_bessel_i0(beta), c = 2.0 * f / rate;
    std::vector<double> g(taps);
    double sum = 0;
    for (uint32_t k = 0; k < taps; k++) {
        const double d = (double)k - (double)H, u = d / (double)H;
        g[k] = c * fir_sinc_pi(c * d) * fir_bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
        sum += g[k];
    }
    for (uint32_t k = 0; k < taps; k++) g[k] /= sum;
    return g;
}

bool fir_design(uint32_t kind, uint32_t rate, double f_lo, double f_hi, uint32_t taps, double beta, std::vector<double> &h, std::string &err) {
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    if (kind > FLO_FIR_BANDSTOP) return bad("kind " + std::to_string(kind) + " is not one of FLO_FIR_LOWPASS .. FLO_FIR_BANDSTOP");
    if (!rate) return bad("rate must be non-zero");
    if (taps < 3 || taps > 65535 || !(taps & 1u)) return bad("taps " + std::to_string(taps) + " must be odd, 3 .. 65535");
    if (!(beta >= 0.0 && beta <= 16.0)) return bad("beta must be finite, 0 .. 16");
    const bool use_lo = kind != FLO_FIR_LOWPASS, use_hi = kind != FLO_FIR_HIGHPASS;
    const double nyquist = (double)rate / 2.0;
    if (use_lo && !(f_lo > 0.0 && f_lo < nyquist)) return bad("f_lo must lie between 0 and rate / 2 = " + std::to_string(nyquist) + " Hz, exclusive");
    if (use_hi && !(f_hi > 0.0 && f_hi < nyquist)) return bad("f_hi must lie between 0 and rate / 2 = " + std::to_string(nyquist) + " Hz, exclusive");
    if (use_lo && use_hi && !(f_lo < f_hi)) return bad("f_lo must be below f_hi");
    const uint32_t H = taps / 2;
    if (kind == FLO_FIR_LOWPASS) {
        h = fir_lowpass(f_hi, rate, taps, beta);
    } else if (kind == FLO_FIR_HIGHPASS) {
        h = fir_lowpass(f_lo, rate, taps, beta);
        for (uint32_t k = 0; k < taps; k++) h[k] = (k == H ? 1.0 : 0.0) - h[k];
    } else {
        h = fir_lowpass(f_hi, rate, taps, beta);
        const std::vector<double> lo = fir_lowpass(f_lo, rate, taps, beta);
        for (uint32_t k = 0; k < taps; k++) h[k] -= lo[k];
        if (kind == FLO_FIR_BANDSTOP)
            for (uint32_t k = 0; k < taps; k++) h[k] = (k == H ? 1.0 : 0.0) - h[k];
    }
    return true;
}

extern "C" int flo_fir_design(uint32_t kind, uint32_t rate, double f_lo, double f_hi, uint32_t taps, double beta, float **table, char *err,
                              size_t err_cap) {
    auto put = [&](const std::string &m) {
        if (err && err_cap) {
            const size_t n = m.size() < err_cap - 1 ? m.size() : err_cap - 1;
            memcpy(err, m.data(), n);
            err[n] = 0;
        }
    };
    if (table) *table = nullptr;
    if (!table) {
        put("table is NULL");
        return FLO_ERR_ARG;
    }
    std::vector<double> h;
    std::string m;
    if (!fir_design(kind, rate, f_lo, f_hi, taps, beta, h, m)) {
        put(m);
        return FLO_ERR_ARG;
    }
    float *t = (float *)malloc(h.size() * sizeof(float));
    if (!t) {
        put("out of memory");
        return FLO_ERR_NOMEM;
    }
    for (size_t k = 0; k < h.size(); k++) t[k] = (float)h[k];
    *table = t;
    return FLO_OK;
}

}  // namespace flo
