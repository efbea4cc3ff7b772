// chroma_siting_check - runs handbrake_amd/csrc/chroma_siting.h (the siting rule crop/scale and colorspace share) on the
// HOST and prints what it gives; tests/test_chroma_siting_cpu.py holds it to tests/chroma_siting_model.py.
//   chroma_siting_check <loc> <log2_cw> <log2_ch> <src_w> <dst_w> <src_h> <dst_h>  [the same seven again ...]
// prints one line per group of seven: `<valid> <shift_x> <shift_y> <h_centred> <v_cosited>` (shifts with 17 digits).
#include "chroma_siting.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 8 || (argc - 1) % 7)
    {
        fprintf(stderr, "usage: chroma_siting_check <loc> <log2_cw> <log2_ch> <src_w> <dst_w> <src_h> <dst_h> ...\n");
        return 1;
    }
    for (int i = 1; i < argc; i += 7)
    {
        const int loc = atoi(argv[i]), lw = atoi(argv[i + 1]), lh = atoi(argv[i + 2]);
        const int sw = atoi(argv[i + 3]), dw = atoi(argv[i + 4]), sh = atoi(argv[i + 5]), dh = atoi(argv[i + 6]);
        if (sw < 1 || dw < 1 || sh < 1 || dh < 1) { fprintf(stderr, "sizes from 1 on\n"); return 1; }
        printf("%d %.17g %.17g %d %d\n", chroma_loc_valid(loc) ? 1 : 0, chroma_resize_shift_x(loc, lw, sw, dw),
               chroma_resize_shift_y(loc, lh, sh, dh), chroma_convert_h_centred(loc) ? 1 : 0, chroma_convert_v_cosited(loc) ? 1 : 0);
    }
    return 0;
}
