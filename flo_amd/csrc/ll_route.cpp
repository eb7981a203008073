// ll_route.cpp — see ll_route.hpp.
#include "ll_route.hpp"

#include <cstring>

LlRoute ll_route(const LlChannelDev &d, bool force_serial) {
    LlRoute r;
    const bool rice = d.len > 0 && (d.n_coeffs > 0 || d.shift_bits >= 128);
    long long csum = 0;
    for (unsigned q = 0; q < d.n_coeffs; q++) csum += d.coeffs[q] < 0 ? -(long long)d.coeffs[q] : (long long)d.coeffs[q];
    bool ser = force_serial || (rice && d.rice_k > kRiceMaxK) || csum >= (1ll << 21) || (d.n_coeffs && (d.shift_bits & 63u) > 20u);
    if (rice && d.len > 16u * 1024u * (unsigned)kRiceTileBits) ser = true;
    r.serial = ser ? 1 : 0;
    r.other = !(d.n_coeffs > 0 && d.n_coeffs <= 12 && d.len > 0 && d.samples > d.n_coeffs) ? 1 : 0;
    r.tiles = rice && !ser ? (d.len + (unsigned)kRiceTileBits / 8u - 1u) / ((unsigned)kRiceTileBits / 8u) : 0u;
    return r;
}

LlChannelDev ll_channel(uint64_t off, uint32_t len, uint8_t n_coeffs, uint8_t shift_bits, uint8_t rice_k, const int32_t *coeffs) {
    LlChannelDev d{};
    d.off = off;
    d.len = len;
    d.n_coeffs = n_coeffs;
    d.shift_bits = shift_bits;
    d.rice_k = rice_k;
    memcpy(d.coeffs, coeffs, sizeof d.coeffs);
    return d;
}

void LlWrapperList::clear() {
    chs.clear();
    tile0.assign(1, 0u);
    serial.clear();
    others.clear();
    frs.clear();
    scratch = 0;
    max_tiles = max_samples = 0;
}

unsigned LlWrapperList::push(const LlChannelDev &d, const LlRoute &r) {
    const unsigned i = (unsigned)chs.size();
    chs.push_back(d);
    chs.back().out_off = scratch;
    scratch += d.samples;
    serial.push_back(r.serial);
    if (r.other) others.push_back(i);
    tile0.push_back(tile0.back() + r.tiles);
    if (r.tiles > max_tiles) max_tiles = r.tiles;
    return i;
}
