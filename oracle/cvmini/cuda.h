/* cvmini: the reference header includes <cuda.h> and uses nothing from it. */
#ifndef CVMINI_CUDA_H_
#define CVMINI_CUDA_H_
#endif
