// What the decode-attention kernels (attn_decode.hip) and their torch
// binding (ext.cpp) must agree on: the chunk geometry that sizes the scratch
// tensors, and the two entry points.
#pragma once

#include <hip/hip_runtime.h>

#define DEC_CHUNK 256       // keys per workgroup pass (DEC_WAVES x 64)
#define DEC_MAX_CHUNKS 128  // chunks per sequence: 32768-token contexts

extern "C" {
// Z chunk-walkers per (b, kvh) and whether the fused scores + PV kernel
// runs; the caller sizes the scratch from these.
void attn_decode_plan(int B, int nkv, int hd, int C, int fp8, int path,
                      int max_z, int* Z_out, int* fused_out);
void launch_attn_decode(
    const unsigned short* q, const void* k_cache, const void* v_cache,
    const int* block_table, const int* seq_lens, unsigned short* p_buf,
    float* part_o, float* part_ml, unsigned short* out, float* out_ml, int B,
    int nkv, int G, int W, int bs, int hd, int C, long q_stride, float scale,
    int fp8, const float* k_scale, const float* v_scale, int window, int path,
    int max_z, hipStream_t stream);
}
