// stamps_dev.hpp -- what a difference of the reference's date_t / time_t means, shared by ema.hip (aqg_decay_from_times) and
// range_window.hip (time-range windows): days of a civil date (proleptic Gregorian) / milliseconds of a time of day.
#pragma once
#include "dev_common.hpp"

namespace {
struct ema_date { unsigned char day, month; short year; };
struct ema_time { unsigned int ms; unsigned char seconds, minutes, hours, pad; };
__device__ inline int64_t stamp_of(ema_date t) {
    const int64_t y = (int64_t)t.year - (t.month <= 2), m = t.month, dd = t.day;
    const int64_t era = (y >= 0 ? y : y - 399) / 400, yoe = y - era * 400;
    const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + dd - 1, doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe;
}
__device__ inline int64_t stamp_of(ema_time t) { return (((int64_t)t.hours * 60 + t.minutes) * 60 + t.seconds) * 1000 + t.ms; }
} // namespace
