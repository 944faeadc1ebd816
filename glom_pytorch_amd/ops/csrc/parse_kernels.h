#pragma once
#include <hip/hip_runtime.h>

// largest patch grid (H*W cells) one parse workgroup holds in LDS; equal to
// ISLAND_MAX_CELLS, and the 10-bit fields of the vote key rely on it
#define PARSE_MAX_CELLS 1024

// labels (PL, N) i32 with PL = P * L -> parents, overlap (PL, N) i32
void launch_island_parents(const int* labels, int* parents, int* overlap,
                           long PL, int L, int N, hipStream_t s);
// levels (P, N, L, D) bf16, labels (P, L, N) i32 -> out (P, N, L, D) f32 or
// bf16 (out_bf16); every row of out is written
void launch_island_means(const void* levels, const int* labels, void* out,
                         long P, int N, int L, int D, bool broadcast,
                         bool out_bf16, hipStream_t s);
