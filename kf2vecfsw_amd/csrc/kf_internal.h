// kf_internal.h -- shared helpers of the kf2vec_gpu library (not part of the ABI).
#pragma once
#include <mutex>
#include <stdint.h>

#include "../../include/kf2vec_gpu.h"

// Records the thread-local error message and returns `code`.
int kf_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Reverse complement of a k-mer in lexicographic code (A0 C1 G2 T3; kf_host.cpp).
uint64_t std_rc(uint64_t x, int k);
