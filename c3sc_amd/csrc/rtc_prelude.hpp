// rtc_prelude.hpp -- what the kernel headers take from the C/C++ standard headers, for run-time compilation (hipRTC,
// rtc.hip).  hipRTC has no <stdint.h>, <stddef.h> or <type_traits>; the headers include this file instead when
// __HIPCC_RTC__ is defined, and hipcc never sees it.  Keep every such stand-in here.
#pragma once
#ifdef __HIPCC_RTC__

typedef __INT8_TYPE__ int8_t;
typedef __INT16_TYPE__ int16_t;
typedef __INT32_TYPE__ int32_t;
typedef __INT64_TYPE__ int64_t;
typedef __UINT8_TYPE__ uint8_t;
typedef __UINT16_TYPE__ uint16_t;
typedef __UINT32_TYPE__ uint32_t;
typedef __UINT64_TYPE__ uint64_t;
typedef __SIZE_TYPE__ size_t;

namespace std {
template <class T, T v>
struct integral_constant {
    static constexpr T value = v;
    typedef T value_type;
    typedef integral_constant type;
    constexpr operator value_type() const noexcept { return value; }
    constexpr value_type operator()() const noexcept { return value; }
};
typedef integral_constant<bool, true> true_type;
typedef integral_constant<bool, false> false_type;
} // namespace std

#endif
