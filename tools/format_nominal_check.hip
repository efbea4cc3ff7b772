// format_nominal_check - runs handbrake_amd/csrc/sws_filter.h's sws_nominal (the tables format.hip's scaler kernels read)
// on the HOST and prints what it builds; tests/test_format_nominal_cpu.py holds it to tests/format_resample_model.py.
//   format_nominal_check <src> <dst> <one> <src_pos> <dst_pos> down|up
// prints `declined`, or `<taps> <group> <base>` and then one line per target sample: the coefficients of its window.
#include "sws_filter.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    if (argc != 7 || (strcmp(argv[6], "down") && strcmp(argv[6], "up")))
    {
        fprintf(stderr, "usage: format_nominal_check <src> <dst> <one> <src_pos> <dst_pos> down|up\n");
        return 1;
    }
    const int src = atoi(argv[1]), dst = atoi(argv[2]);
    if (src < 1 || dst < 1) { fprintf(stderr, "sizes from 1 on\n"); return 1; }
    const SwsNominalFrame &fr = strcmp(argv[6], "up") ? SWS_NOMINAL_DOWN : SWS_NOMINAL_UP;
    std::vector<short> q;
    if (!sws_nominal(src, dst, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), 1, fr, q)) { puts("declined"); return 0; }
    printf("%d %d %d\n", fr.taps, fr.group, fr.base);
    for (int i = 0; i < dst; i++)
        for (int k = 0; k < fr.taps; k++) printf("%d%c", q[(size_t)i * fr.taps + k], k + 1 < fr.taps ? ' ' : '\n');
    return 0;
}
