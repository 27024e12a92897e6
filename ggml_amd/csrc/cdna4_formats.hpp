// cdna4_formats.hpp — host-side helpers of the launchers: the weight formats at run time (two lists, one dispatcher, accessors that read QT<> of
// cdna4_common.h through it) and the dynamic-LDS limit of a kernel.  Kernel-library sources only: not one of the .h / .inc files the ggml plug-in's
// checksum covers (ggml_amd/build.py), which name everything the plug-in's build can depend on.
#pragma once
#include "cdna4_common.h"
#include <type_traits>

template <int... T> struct cdna4_types {};
typedef cdna4_types<CDNA4_Q4_0, CDNA4_Q4_1, CDNA4_Q5_0, CDNA4_Q5_1, CDNA4_Q8_0, CDNA4_Q2_K, CDNA4_Q3_K, CDNA4_Q4_K, CDNA4_Q5_K, CDNA4_Q6_K, CDNA4_IQ4_NL, CDNA4_IQ4_XS> cdna4_all12;
typedef cdna4_types<CDNA4_Q4_K, CDNA4_Q5_K, CDNA4_Q6_K, CDNA4_Q4_0, CDNA4_Q8_0> cdna4_main5;      // the formats with matrix-core and multi-row forms of their own
// f(std::integral_constant<int, T>{}) for the T of the list that equals `type`; false (f not called): `type` is not in the list — the caller's own error.
// Only the listed T are instantiated.
template <int... T, typename F> inline bool cdna4_dispatch(cdna4_types<T...>, int type, F &&f) {
    return ((type == T && (f(std::integral_constant<int, T>{}), true)) || ...);
}
inline int cdna4_type_qk(int type) { int v = 0; cdna4_dispatch(cdna4_all12{}, type, [&](auto t) { v = QT<t.value>::QK; }); return v; }        // weights per block; 0: not a quantized weight format
inline int cdna4_type_bytes(int type) { int v = 0; cdna4_dispatch(cdna4_all12{}, type, [&](auto t) { v = QT<t.value>::BYTES; }); return v; }  // bytes per block (0 likewise)
inline bool cdna4_type_is_kq(int type) { return cdna4_type_qk(type) == QK_K; }                                                                // a 256-weight superblock format
inline bool cdna4_type_is_main5(int type) { return cdna4_dispatch(cdna4_main5{}, type, [](auto) {}); }

// raise the dynamic-LDS limit of KERNELS (launched together by one launcher) to `bytes`, once per device: a function attribute is per device, so the flag is too
// (a device outside 0..15 shares slot 0).  0, or the error status with the caller's message
template <auto... KERNELS> inline int cdna4_raise_lds_limit(int bytes, const char *msg) {
    static bool raised_[16] = {};
    int dev = 0; if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); dev = 0; }
    if (raised_[dev]) return 0;
    if (((hipFuncSetAttribute((const void *)KERNELS, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) || ...)) { (void)hipGetLastError(); return cdna4_set_error_msg(msg); }
    raised_[dev] = true;
    return 0;
}
