// A byte as a model-normalised value: ToTensor + Normalize, (b / 255 - mean) / std in the reference's order - an IEEE division, a
// subtraction and an IEEE division, each rounded on its own (the empty asm keeps the compiler from merging the two divisors).  Shared by
// elementwise.hip (pbe_u8_to_planes_f32) and exemplar.hip (the planes of pbe_resample_v_u8): one definition, so the bits agree.
#pragma once

__device__ __forceinline__ float pbe_u8_norm(unsigned char b, float mean, float sd) {
    float v = (float)b / 255.0f;
    v = v - mean;
    asm volatile("" : "+v"(v));
    return v / sd;
}
