// dirmap_vote_check.hip - handbrake_amd/csrc/eedi2_dirmap_vote.h, the text the dir-map kernels are compiled from, run on the
// HOST for tests/test_dir_map_vote_cpu.py (no GPU is touched).  Results go to stdout as text, one case per line.
//   ranks           every assignment of { 0, 1, absent } to the nine slots: "s1 s2 s3 s4" of dmv_ranks1to4 (columns sorted first)
//   avg             dmv_vote_avg(a, b) for a = 0 .. 2559, b = 1 .. 10
//   quad <file>     the file holds cases of nine little-endian dwords (u0 u1 u2 c0 c1 c2 d0 d1 d2): per case the result of
//                   dir_map_quad<3>, of <1> and of <2>, and the peaks of the pairs (0, 1) and (2, 3) as dmv_unpack counts them
// build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -fno-fast-math -Ihandbrake_amd/csrc tools/dirmap_vote_check.hip -o tools/dirmap_vote_check
#include "eedi2_dirmap_vote.h"
#include <cstdio>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "ranks"))
    {
        const uint32_t val[3] = { 0, 1, DMV_ABSENT };
        for (int c = 0; c < 19683; c++)
        {
            dmv_h2 v[9];
            for (int i = 0, t = c; i < 9; i++, t /= 3) v[i] = dmv_pk1(val[t % 3]);
            for (int k = 0; k < 9; k += 3) { dmv_cswap(v[k], v[k + 1]); dmv_cswap(v[k + 1], v[k + 2]); dmv_cswap(v[k], v[k + 1]); }
            dmv_h2 s1, s2, s3, s4;
            dmv_ranks1to4(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], s1, s2, s3, s4);
            printf("%u %u %u %u\n", dmv_un(s1) & 0xffffu, dmv_un(s2) >> 16, dmv_un(s3) & 0xffffu, dmv_un(s4) >> 16);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "avg"))
    {
        for (int a = 0; a < 2560; a++)
            for (int b = 1; b <= 10; b++) printf("%d\n", dmv_vote_avg(a, b));
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "quad"))
    {
        FILE *f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
        uint32_t w[9];
        while (fread(w, 4, 9, f) == 9)
        {
            const uint32_t rows[3][3] = { { w[0], w[1], w[2] }, { w[3], w[4], w[5] }, { w[6], w[7], w[8] } };
            dmv_h2 X[3], Y[3], Z[3];
            uint32_t aX, aY, aZ;
            dmv_unpack(rows, X, Y, Z, aX, aY, aZ);
            printf("%u %u %u %u %u\n", dir_map_quad<3>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]),
                   dir_map_quad<1>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]),
                   dir_map_quad<2>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]),
                   dmv_pair_absent(aX, aY), dmv_pair_absent(aY, aZ));
        }
        fclose(f);
        return 0;
    }
    fprintf(stderr, "usage: dirmap_vote_check ranks | avg | quad <file>\n");
    return 2;
}
