// segments.h -- which segment an element belongs to: the image of a key point, the pair of a match row, the voxel of a map point,
// the component of an observation, the frame of a scan point.  The one search of the front ends over ascending segment offsets
// (match.hip, verify.hip, resect.hip, fusion.hip, track_graph.hip; scan_points.h and track_graph_device.h forward to it).  Host/device-neutral,
// integer-only, no HIP includes: also compiled by g++ (tests/segments_check.cpp).  The lower-bound searches for a KEY
// (voxel_lookup.h, tg_lower_bound, ...) are a different primitive.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define LVBA_SEG_HD __host__ __device__ __forceinline__
#else
#define LVBA_SEG_HD inline
#endif

namespace lvba {

// key(s) of an offset array is off[s]; of anything else, what calling it with s gives (jobs[s].first, off[s] - off[0], ...)
template <class T, class I> LVBA_SEG_HD T seg_key(const T *off, I s) { return off[s]; }
template <class F, class I> LVBA_SEG_HD auto seg_key(const F &key, I s) -> decltype(key(s)) { return key(s); }

// The last s in [0, n) with key(s) <= i, for n >= 1 segments with ascending keys and key(0) <= i.  Segment s holds the elements
// key(s) <= i < key(s + 1); an EMPTY segment shares its key with its successor, so of all segments whose key is <= i only the
// last can hold i -- "last" steps over images without key points, pairs without matches and frames without points, at the
// start, in the middle and in a row.  key(n) is never read.  I is the index type of the caller's loop (32 or 64 bits).
template <class I, class K, class X> LVBA_SEG_HD I segment_of(const K &key, I n, X i)
{
    I lo = 0, hi = n;
    while (hi - lo > 1) {
        const I mid = (lo + hi) >> 1;
        if (seg_key(key, mid) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

} // namespace lvba
