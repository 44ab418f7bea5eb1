// The two users of fft_three_stage.h, compiled as ONE translation unit: lens_fft.hip (the padded lens convolution) and
// cube_fft.hip (3-D transforms of float64 and side-2048 fp32 cubes).  Each source stands alone and compiles alone, but the
// compiler settles the argument ranges of the file-local device functions (three_stage, fft_reg) from all their callers in
// the unit: compiled apart, the fifteen lens row kernels of 128 ... 2048 points come out with other address arithmetic
// than compiled together (scripts/kernel_asm_digest.py; profiles/EXPERIMENTS.md).  Together they are the code that was
// measured, and there is one float64 twiddle cache instead of two.
#include "lens_fft.hip"
#include "cube_fft.hip"
