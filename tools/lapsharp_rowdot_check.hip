// lapsharp_rowdot_check - runs handbrake_amd/csrc/lapsharp_rowdot.h (the arithmetic of lapsharp3_wide_kernel) on the HOST
// and writes what it computes; tests/test_lapsharp_rowdot_cpu.py holds the expectations, written out independently.
//   rows <a> <b> <c> <out>       for every window l | m << 8 | r << 16 (2^24), with a fourth byte that must not count:
//                                one uint32 U | H << 16
//   quad <a> <b> <c> <kinv> <mixf bits> <in> <out>
//                                <in>: windows of 3 rows x 3 dwords (columns x - 4 .. x + 7); per window and pixel 0 .. 3 two
//                                int32: the nine-tap accumulator and the one-float-multiply mix's output sample
//   window                       prints lrd_window<4>(ext, p), p = 0 .. 15, for ext = the bytes 0 .. 23
#include "lapsharp_rowdot.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool taps_of(char **argv, LrdTaps &t)
{
    if (lrd_taps(atoi(argv[0]), atoi(argv[1]), atoi(argv[2]), t)) return true;
    fprintf(stderr, "not a table of the header's shape\n");
    return false;
}

int main(int argc, char **argv)
{
    LrdTaps t;
    if (argc == 6 && !strcmp(argv[1], "rows"))
    {
        if (!taps_of(argv + 2, t)) return 2;
        std::vector<uint32_t> out(1u << 24);
        for (uint32_t w = 0; w < (1u << 24); w++)
        {
            const uint32_t win = w | ((w * 2654435761u) & 0xff000000u);
            out[w] = lrd_row_u(win, t) | (lrd_row_h(win, t) << 16);
        }
        FILE *f = fopen(argv[5], "wb");
        if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
        fclose(f);
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "quad"))
    {
        if (!taps_of(argv + 2, t)) return 2;
        const int kinv = atoi(argv[5]);
        const uint32_t mbits = (uint32_t)strtoul(argv[6], nullptr, 0);
        float mixf;
        memcpy(&mixf, &mbits, 4);
        const float ckf = (float)(t.c - kinv);
        FILE *f = fopen(argv[7], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[7]); return 2; }
        std::vector<int32_t> out;
        uint32_t w[3][3];
        while (fread(w, 4, 9, f) == 9)
        {
            uint32_t u[3][4], h[4];
            for (int r = 0; r < 3; r++)
                for (int p = 0; p < 4; p++)
                {
                    const uint32_t win = lrd_window<1>(w[r], p);
                    u[r][p] = lrd_row_u(win, t);
                    if (r == 1) h[p] = lrd_row_h(win, t);
                }
            const uint32_t own = w[1][1];
            const float mix[4] = { lrd_mix_fast<0>(own, lrd_neg_sum(h[0], u[0][0], u[2][0]), ckf, mixf),
                                   lrd_mix_fast<1>(own, lrd_neg_sum(h[1], u[0][1], u[2][1]), ckf, mixf),
                                   lrd_mix_fast<2>(own, lrd_neg_sum(h[2], u[0][2], u[2][2]), ckf, mixf),
                                   lrd_mix_fast<3>(own, lrd_neg_sum(h[3], u[0][3], u[2][3]), ckf, mixf) };
            for (int p = 0; p < 4; p++)
            {
                out.push_back(lrd_acc((int)((own >> (8 * p)) & 0xffu), lrd_neg_sum(h[p], u[0][p], u[2][p]), t));
                out.push_back((int32_t)lrd_sat_u8(mix[p]));
            }
        }
        fclose(f);
        f = fopen(argv[8], "wb");
        if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[8]); return 2; }
        fclose(f);
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "window"))
    {
        uint32_t ext[6];
        for (int j = 0; j < 6; j++) ext[j] = 0x03020100u + 0x04040404u * (uint32_t)j;
        for (int p = 0; p < 16; p++) printf("%u\n", lrd_window<4>(ext, p));
        return 0;
    }
    fprintf(stderr, "usage: lapsharp_rowdot_check rows <a> <b> <c> <out> | quad <a> <b> <c> <kinv> <mixf bits> <in> <out> | window\n");
    return 1;
}
