// The letterbox of one source image (Model.predict): the record k_letterbox (image_prep.hip) places the image by and
// k_rows_to_source (decode_nms.hip) maps the detections back by.  Filled and checked by yolo_letter_fill only.
#pragma once

// source (uint8 HWC, H x W, at byte `off` of the source buffer) resized to (nh, nw) and placed at (left, top) on the S x S
// canvas; (sx, sy) = (W / nw, H / nh), each the double quotient rounded once to fp32: the per-axis map back (the resize goes
// to an integer size, so the per-axis ratio, not one common gain, is its exact inverse).  nw = nh = 0 is the blank slot: all
// fill, no source read
struct LetterRec { long off; int H, W; int nw, nh; int left, top; float sx, sy; };
