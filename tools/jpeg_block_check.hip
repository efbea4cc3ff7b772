// jpeg_block_check - runs handbrake_amd/csrc/jpeg_block.h (the arithmetic of the preview JPEG's kernels, jpeg.hip) on the
// HOST; tests/test_preview_jpeg_cpu.py compares what it prints with tests/jpeg_model.py.
//   jpeg_block_check [file]     reads from the file, or from stdin: the text "<width> <height> <quality>\n", then the Y, Cb
//                               and Cr planes of an 8-bit 4:2:0 picture, rows packed
// It prints a line per block of the scan, in coding order:
//   <component> <dummy 0|1> <64 coefficients in scan order> <bit string>
// A dummy block prints zeros behind the DC it inherits.
#include "jpeg_block.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

struct StringSink
{
    std::string bits;
    void put(uint32_t code, int n)
    {
        for (int i = n - 1; i >= 0; i--) bits.push_back((code >> i) & 1u ? '1' : '0');
    }
};

int main(int argc, char **argv)
{
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : stdin;
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int width = 0, height = 0, quality = 0;
    if (fscanf(f, "%d %d %d", &width, &height, &quality) != 3 || fgetc(f) != '\n' || width < 2 || height < 2 ||
        ((width | height) & 1) || width > 16384 || height > 16384 || quality < 1 || quality > 100)
    {
        fprintf(stderr, "usage: jpeg_block_check [file]   (\"<even width> <even height> <quality 1..100>\\n\", then the three planes)\n");
        return 1;
    }
    const JpbGeom g = jpb_geom(width, height);
    // planes with rows of a multiple of 16 bytes, as jpb_load_block reads them
    std::vector<uint8_t> plane[3];
    int pitch[3], pw[3], ph[3];
    for (int c = 0; c < 3; c++)
    {
        pw[c] = c ? width / 2 : width; ph[c] = c ? height / 2 : height;
        pitch[c] = (pw[c] + 15) / 16 * 16;
        plane[c].assign((size_t)pitch[c] * ph[c], 0);
        for (int y = 0; y < ph[c]; y++)
            if (fread(plane[c].data() + (size_t)y * pitch[c], 1, pw[c], f) != (size_t)pw[c])
            {
                fprintf(stderr, "short input\n");
                return 2;
            }
    }
    JpbTables t;
    jpb_tables(quality, &t);
    const int blocks = 6 * g.mcus_w * g.mcus_h;
    std::vector<int16_t> zz((size_t)64 * blocks, 0);
    for (int b = 0; b < blocks; b++)
    {
        const JpbPlace p = jpb_place(g, b);
        if (p.dummy) continue;
        int d[64];
        jpb_load_block(plane[p.comp].data(), pitch[p.comp], pw[p.comp], ph[p.comp], p.bx, p.by, d);
        jpb_transform_block(d, t.divisor[p.comp != 0], &zz[(size_t)64 * b]);
    }
    for (int b = 0; b < blocks; b++)
    {
        const JpbPlace p = jpb_place(g, b);
        const int tb = p.comp != 0;
        const int from = jpb_pred_block(g, b);
        const int pred = from < 0 ? 0 : zz[(size_t)64 * from];
        const int16_t *z = &zz[(size_t)64 * b];
        StringSink sink;
        if (p.dummy) jpb_code_dummy(t.dc[tb], t.ac[tb], sink);
        else jpb_code_block([z](int k) { return (int)z[k]; }, pred, t.dc[tb], t.ac[tb], sink);
        printf("%d %d", p.comp, p.dummy ? 1 : 0);
        for (int k = 0; k < 64; k++) printf(" %d", p.dummy ? (k ? 0 : pred) : z[k]);
        printf(" %s\n", sink.bits.c_str());
    }
    return 0;
}
