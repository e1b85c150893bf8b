// bcp_outline.h -- the OUTLINE runs of one polygon edge as cv2.fillPoly draws them (the head of bcp_raster.h states the
// rule).  Plain C++ with no HIP in it: the footprint rasteriser (bcp_raster.h) and the box sampler (bcp_boxes_cell.h, on the
// device and in its host program) walk edges through this one function.
#pragma once

#include "bcp_philox.h"   // BCP_HD_INLINE

namespace bcp {

// OUTLINE runs of edge (x0,y0)->(x1,y1): cv::LineIterator(pt0, pt1, connectivity 8, leftToRight = true).
// Returns true when the sink asked to stop.
template <typename Sink>
BCP_HD_INLINE bool outline_edge(int x0, int y0, int x1, int y1, Sink& sink)
{
    int sx = x0, sy = y0, dx = x1 - x0, dy = y1 - y0;
    if (dx < 0) {  // start from the end point with the smaller x
        dx = -dx;
        dy = -dy;
        sx = x1;
        sy = y1;
    }
    int ystep = 1;
    if (dy < 0) {
        dy = -dy;
        ystep = -1;
    }
    bool stop = false;
    if (dy > dx) {
        // y-major: one pixel per row, x = sx + floor((2*dx*i + dy - 1) / (2*dy))  (minor step when err < 0)
        int rem = dy - 1, q = 0;
        const int two_d = 2 * dx, two_D = 2 * dy;
        int yy = sy;
        for (int i = 0; i <= dy; ++i) {
            if (!stop) stop = sink.pixel(yy, sx + q);
            rem += two_d;
            if (rem >= two_D) {
                rem -= two_D;
                ++q;
            }
            yy += ystep;
        }
    } else if (dy == 0) {
        stop = sink.span(sy, sx, sx + dx);  // horizontal edge or single point
    } else {
        // x-major: row j holds steps i in [lo, hi], hi(j) = min(dx, floor((2*dx*j + dx) / (2*dy))), lo(j) = hi(j-1)+1
        const int two_d = 2 * dy;
        const int qs = (2 * dx) / two_d, rs = (2 * dx) - qs * two_d;
        int q = dx / two_d, rem = dx - q * two_d;
        int lo = 0, yy = sy;
        for (int j = 0; j <= dy; ++j) {
            const int hi = q > dx ? dx : q;
            if (!stop) stop = sink.span(yy, sx + lo, sx + hi);
            lo = hi + 1;
            q += qs;
            rem += rs;
            if (rem >= two_d) {
                rem -= two_d;
                ++q;
            }
            yy += ystep;
        }
    }
    return stop;
}

}  // namespace bcp
