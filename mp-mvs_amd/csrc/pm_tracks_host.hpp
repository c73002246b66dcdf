// pm_tracks_host.hpp -- the host end of the fusion's tracks (pm_fusion.hpp, include/mpmvs.h): three malloc'ed arrays that grow
// image by image while the device buffers, which hold ONE image's tracks, are reused.  Host code only (no HIP): the
// stand-alone check tools/track_sink_check.cpp drives it under the address and undefined-behaviour sanitizers.
//   off    one entry per point plus one: off[p] = index of point p's first entry, off[points] = entries
//   image  per entry the image index          pixel  per entry the raster index in that image
// Per image: reserve(points, entries) makes room, the caller copies the image's offsets to off_tail() and its entries to
// image_tail() / pixel_tail(), commit(points, entries) makes them part of the result.  finish() closes the offsets and hands
// the arrays over (release with free); without finish() the destructor frees them.
#pragma once

#include <cstdint>
#include <cstdlib>

namespace pm {

class TrackSink {
    long long* off_ = nullptr;
    int32_t* image_ = nullptr;
    int32_t* pixel_ = nullptr;
    size_t points_ = 0, entries_ = 0, cap_off_ = 0, cap_image_ = 0, cap_pixel_ = 0;

    // capacity for `need` elements: at least doubled, so that n images cost O(total) copying
    template <typename T>
    static bool grow(T*& p, size_t& cap, size_t need) {
        if (need <= cap) return true;
        const size_t want = cap * 2 > need ? cap * 2 : need;
        if (want > SIZE_MAX / sizeof(T)) return false;
        T* q = (T*)std::realloc(p, want * sizeof(T));
        if (!q) return false;
        p = q;
        cap = want;
        return true;
    }

   public:
    TrackSink() = default;
    TrackSink(const TrackSink&) = delete;
    TrackSink& operator=(const TrackSink&) = delete;
    ~TrackSink() {
        std::free(off_);
        std::free(image_);
        std::free(pixel_);
    }
    size_t points() const { return points_; }
    size_t entries() const { return entries_; }
    // room for `points` more points (and the closing offset) and `entries` more entries; false: no memory (what is there stays valid)
    bool reserve(size_t points, size_t entries) {
        if (points > SIZE_MAX - points_ - 1 || entries > SIZE_MAX - entries_) return false;
        return grow(off_, cap_off_, points_ + points + 1) && grow(image_, cap_image_, entries_ + entries) && grow(pixel_, cap_pixel_, entries_ + entries);
    }
    long long* off_tail() { return off_ + points_; }
    int32_t* image_tail() { return image_ + entries_; }
    int32_t* pixel_tail() { return pixel_ + entries_; }
    // false: what was copied in does not continue the arrays (first offset != entries so far)
    bool commit(size_t points, size_t entries) {
        if (points_ + points + 1 > cap_off_ || entries_ + entries > cap_image_ || entries_ + entries > cap_pixel_) return false;
        if (points && off_[points_] != (long long)entries_) return false;
        points_ += points;
        entries_ += entries;
        return true;
    }
    // closes the offsets; the caller owns the three arrays from here on.  false: no memory (nothing handed over)
    bool finish(long long** off, int32_t** image, int32_t** pixel) {
        if (!reserve(0, 0)) return false;
        if (!image_ && !(image_ = (int32_t*)std::malloc(sizeof(int32_t)))) return false;   // an empty cloud still returns buffers to free
        if (!pixel_ && !(pixel_ = (int32_t*)std::malloc(sizeof(int32_t)))) return false;
        off_[points_] = (long long)entries_;
        *off = off_;
        *image = image_;
        *pixel = pixel_;
        off_ = nullptr;
        image_ = pixel_ = nullptr;
        points_ = entries_ = cap_off_ = cap_image_ = cap_pixel_ = 0;
        return true;
    }
};

}  // namespace pm
