#pragma once
#include <hip/hip_runtime.h>

// largest patch grid (H*W cells) one labelling workgroup holds in LDS
#define ISLAND_MAX_CELLS 1024

void launch_island_dots(const void* levels, float* norm, float* out, long P,
                        int H, int W, int L, int D, int C, hipStream_t s);
void launch_island_finish(const float* norm, float* out, long PL, int H,
                          int W, int C, hipStream_t s);
void launch_island_labels(const float* agreement, int* labels, long PL,
                          int H, int W, int C, float threshold,
                          hipStream_t s);
void launch_island_sizes(const int* labels, int* sizes, int* count, long PL,
                         int N, hipStream_t s);
