// The two pictures of the tone matching as BYTES - the grey levels the paste writes.  Shared by tone.hip (the moment sums) and
// tone_field.hip (the cell sums): one definition, so that the two tables count the same bytes.  tests/toneref.py restates them.
#pragma once

__device__ __forceinline__ float tone_c01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }          // fmaxf(NaN, 0) = 0: a NaN counts as 0
// the byte of a model-normalised value.  0.5f * x is exact (a power of two), so the sum is rounded once whether or not the compiler
// contracts 0.5f * x + 0.5f into an fma: the two forms agree bit for bit, and tests/toneref.py takes the uncontracted one.
__device__ __forceinline__ unsigned tone_byte_image(float x) { return (unsigned)(int)rintf(255.0f * tone_c01(0.5f * x + 0.5f)); }
__device__ __forceinline__ unsigned tone_byte_result(float r) { return (unsigned)(int)rintf(255.0f * tone_c01(r)); }       // rintf: half to even

template <int VEC> struct ToneVec;
template <> struct ToneVec<1> { typedef float type; };
template <> struct ToneVec<2> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct ToneVec<4> { typedef float type __attribute__((ext_vector_type(4))); };
