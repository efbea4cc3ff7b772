// chroma_siting.h - where a stream's chroma samples sit (AVCHROMA_LOC_*), stated once for the two filters whose
// reference engine is zscale: crop/scale (alias.hip) and colorspace (colorspace.hip).  Host code only.
//
//                    ***  PARITY UNPINNED  ***
// The reference hands each frame's chroma_location to the avfilter graph (hbffmpeg.c:130) and never sets zscale's
// chromal / chromal_in, so zscale takes its input and output siting from that field.  What follows is zimg's
// chroma_shift arithmetic as recalled; neither zimg nor FFmpeg is in the reference tree, and no golden vector pins
// these rows.  tests/chroma_siting_model.py restates them independently; tests/test_chroma_siting_cpu.py also checks
// the direction of the crop/scale shift without the formula (a ramp sampled at the sited positions).
//
//   location        0 unspecified  1 left  2 center  3 topleft  4 top  5 bottomleft  6 bottom
//   horizontally    co-sited       co      centred   co         centred co           centred
//   vertically      centred        centred centred   top        top    bottom        bottom
//
// zimg's raw offset of a direction, in chroma samples of that plane: -0.5 co-sited (left / top), 0 centred, +0.5 bottom.
#pragma once

constexpr int CHROMA_LOC_LEFT = 1, CHROMA_LOC_LAST = 6;

inline bool chroma_loc_valid(int loc) { return loc >= 0 && loc <= CHROMA_LOC_LAST; }

inline bool chroma_h_cosited(int loc) { return loc == 0 || loc == 1 || loc == 3 || loc == 5; }
inline bool chroma_v_top(int loc)     { return loc == 3 || loc == 4; }
inline bool chroma_v_bottom(int loc)  { return loc == 5 || loc == 6; }

inline double chroma_raw_offset_h(int loc) { return chroma_h_cosited(loc) ? -0.5 : 0.0; }
inline double chroma_raw_offset_v(int loc) { return chroma_v_top(loc) ? -0.5 : chroma_v_bottom(loc) ? 0.5 : 0.0; }

// The shift a resize of one direction of a chroma plane gets, in source chroma samples: -raw * 0.5 * (1 - src / dst),
// src and dst the LUMA sizes (cropped, output) of that direction.  Nothing where the direction is not subsampled.
// Left-sited: 0.25 * (1 - src / dst), the one shift there was before the location was honoured.
inline double chroma_resize_shift(double raw, bool subsampled, int src_luma, int dst_luma)
{
    return subsampled ? -raw * 0.5 * (1.0 - (double)src_luma / (double)dst_luma) : 0.0;
}
inline double chroma_resize_shift_x(int loc, int log2_cw, int src_w, int dst_w)
{
    return chroma_resize_shift(chroma_raw_offset_h(loc), log2_cw > 0, src_w, dst_w);
}
inline double chroma_resize_shift_y(int loc, int log2_ch, int src_h, int dst_h)
{
    return chroma_resize_shift(chroma_raw_offset_v(loc), log2_ch > 0, src_h, dst_h);
}

// The colour conversion's up- and down-sampling knows two forms a direction: co-sited and centred.  Vertical "bottom"
// stays centred there (an approximation: INTEGRATION.md section 6), so locations 0, 1 and 5 are one form, 2 and 6 another.
inline bool chroma_convert_h_centred(int loc) { return !chroma_h_cosited(loc); }
inline bool chroma_convert_v_cosited(int loc) { return chroma_v_top(loc); }
