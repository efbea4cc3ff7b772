// sws_filter.h — libswscale's filter table of one dimension, built on the host: the one copy behind the crop/scale and format
// drop-in's swscale branch (alias.hip), the format drop-in's scaler (format.hip) and the bitmap subtitle scaler (blend.hip,
// bitmap_scale.hip).  Host code only: tools/format_nominal_check runs it without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

// libswscale's filter of one dimension for SWS_LANCZOS (utils.c:initFilter), formula for formula as oracle/alias_oracle.c:
// orc_sws_filter states it (same libm, same expression order: the tables come out equal).  Returns the tap count.
// bicubic: SWS_BICUBIC at its default parameters instead (B = 0, C = 0.6: the flags of libavfilter's auto-inserted `scale`;
// the format filter's chroma down-sampling) - its own size factor, 4, and initFilter's integer cubic in d, in units of
// 6 * fone; the normalisation, the cut-off trimming and the edge folding are the same code.
inline int sws_filter(int src, int dst, int one, int src_pos, int dst_pos, std::vector<int> &pos, std::vector<short> &coef,
                      bool bicubic = false)
{
    auto ilog2 = [](unsigned v) { int n = 0; while (v >>= 1) n++; return n; };
    const int64_t fone = 1LL << (54 - std::min(ilog2((unsigned)(src / dst)), 8));
    const int x_inc = (int)((((int64_t)src << 16) + (dst >> 1)) / dst);
    pos.assign((size_t)dst, 0);
    int size;
    std::vector<int64_t> f;
    if (std::llabs((long long)x_inc - 0x10000) < 10 && src_pos == dst_pos)
    {
        size = 1;
        f.assign((size_t)dst, fone);
        for (int i = 0; i < dst; i++) pos[i] = i;
    }
    else
    {
        const int size_factor = bicubic ? 4 : 6;
        size = x_inc <= (1 << 16) ? 1 + size_factor : 1 + (size_factor * src + dst - 1) / dst;
        size = std::max(std::min(size, src - 2), 1);
        f.assign((size_t)dst * size, 0);
        int64_t x_dst_in_src = (((int64_t)dst_pos * x_inc) >> 7) - (((int64_t)src_pos * 0x10000LL) >> 7);
        for (int i = 0; i < dst; i++)
        {
            int xx = (int)((x_dst_in_src - (int64_t)(size - 2) * (1LL << 16)) / (1 << 17));
            pos[i] = xx;
            for (int j = 0; j < size; j++)
            {
                int64_t d = std::llabs(((int64_t)xx * (1 << 17)) - x_dst_in_src) << 13;
                if (x_inc > (1 << 16)) d = d * dst / src;
                const double fd = (double)d * (1.0 / (1 << 30));
                if (bicubic)
                {
                    const int64_t C = (int64_t)(0.6 * (1 << 24)), U = 1LL << 24;          // (B = 0 drops out of both arms)
                    int64_t c = 0;
                    if (d < (1LL << 31))
                    {
                        const int64_t dd = (d * d) >> 30, ddd = (dd * d) >> 30;
                        c = d < (1LL << 30) ? (12 * U - 6 * C) * ddd + (-18 * U + 6 * C) * dd + 6 * U * (1LL << 30)
                                            : -6 * C * ddd + 30 * C * dd - 48 * C * d + 24 * C * (1LL << 30);
                    }
                    f[(size_t)i * size + j] = c / ((1LL << 54) / fone);
                    xx++;
                    continue;
                }
                int64_t c = (int64_t)((d ? std::sin(fd * M_PI) * std::sin(fd * M_PI / 3.0) / (fd * fd * M_PI * M_PI / 3.0) : 1.0) * (double)fone);
                if (fd > 3.0) c = 0;
                f[(size_t)i * size + j] = c;
                xx++;
            }
            x_dst_in_src += 2 * (int64_t)x_inc;
        }
    }
    int min_size = 0;
    const double cut = 0.002 * (double)fone;
    for (int i = dst - 1; i >= 0; i--)
    {
        int64_t *row = &f[(size_t)i * size];
        int mn = size;
        int64_t cut_off = 0;
        for (int j = 0; j < size; j++)
        {
            cut_off += std::llabs(row[0]);
            if ((double)cut_off > cut) break;
            if (i < dst - 1 && pos[i] >= pos[i + 1]) break;
            for (int k = 1; k < size; k++) row[k - 1] = row[k];
            row[size - 1] = 0;
            pos[i]++;
        }
        cut_off = 0;
        for (int j = size - 1; j > 0; j--)
        {
            cut_off += std::llabs(row[j]);
            if ((double)cut_off > cut) break;
            mn--;
        }
        min_size = std::max(min_size, mn);
    }
    const int fsize = min_size;
    std::vector<int64_t> g((size_t)dst * fsize, 0);
    for (int i = 0; i < dst; i++)
        for (int j = 0; j < fsize && j < size; j++) g[(size_t)i * fsize + j] = f[(size_t)i * size + j];
    for (int i = 0; i < dst; i++)
    {
        int64_t *row = &g[(size_t)i * fsize];
        if (pos[i] < 0)
        {
            for (int j = 1; j < fsize; j++)
            {
                const int left = std::max(j + pos[i], 0);
                row[left] += row[j];
                row[j] = 0;
            }
            pos[i] = 0;
        }
        if (pos[i] + fsize > src)
        {
            const int shift = pos[i] + std::min(fsize - src, 0);
            int64_t acc = 0;
            for (int j = fsize - 1; j >= 0; j--)
                if (pos[i] + j >= src) { acc += row[j]; row[j] = 0; }
            for (int j = fsize - 1; j >= 0; j--) row[j] = j < shift ? 0 : row[j - shift];
            pos[i] -= shift;
            row[src - 1 - pos[i]] += acc;
        }
    }
    coef.assign((size_t)dst * fsize, 0);
    for (int i = 0; i < dst; i++)
    {
        const int64_t *row = &g[(size_t)i * fsize];
        int64_t error = 0, sum = 0;
        for (int j = 0; j < fsize; j++) sum += row[j];
        sum = (sum + one / 2) / one;
        if (!sum) sum = 1;
        for (int j = 0; j < fsize; j++)
        {
            const int64_t v = row[j] + error;
            const int64_t iv = v >= 0 ? (v + (sum >> 1)) / sum : -((-v + (sum >> 1)) / sum);
            coef[(size_t)i * fsize + j] = (short)iv;
            error = v - iv * sum;
        }
    }
    return fsize;
}

// The frame the format scaler's kernels read a bicubic table in (format.hip): row i taps the `taps` source samples from
// 2 * (i >> group) + base on - a window that starts on an even sample whatever the row.  Down, 2:1: each row its own
// window of ten; up, 1:2: four adjacent rows share one of six.
struct SwsNominalFrame { int taps, group, base; };
constexpr SwsNominalFrame SWS_NOMINAL_DOWN = { 10, 0, -4 }, SWS_NOMINAL_UP = { 6, 2, -2 };

// sws_filter(bicubic)'s rows moved into that frame, zeros around them, `dst` padded to a multiple of `pad` rows.
// false: a row has a tap outside of its window or of the plane - the kernels cannot take that table.
inline bool sws_nominal(int src, int dst, int one, int src_pos, int dst_pos, int pad, const SwsNominalFrame &fr,
                        std::vector<short> &out)
{
    std::vector<int> pos;
    std::vector<short> coef;
    const int taps = sws_filter(src, dst, one, src_pos, dst_pos, pos, coef, true);
    out.assign((size_t)((dst + pad - 1) / pad * pad) * fr.taps, 0);
    for (int i = 0; i < dst; i++)
        for (int t = 0; t < taps; t++)
        {
            const short q = coef[(size_t)i * taps + t];
            if (q == 0) continue;
            const int k = pos[i] + t - (2 * (i >> fr.group) + fr.base);
            if (k < 0 || k >= fr.taps || pos[i] + t < 0 || pos[i] + t >= src) return false;
            out[(size_t)i * fr.taps + k] = q;
        }
    return true;
}
