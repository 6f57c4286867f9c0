/* cvmini: forwards to opencv2/core.hpp, the one real stand-in header. */
#ifndef CVMINI_OPENCV2_CORE_TYPES_C_H_
#define CVMINI_OPENCV2_CORE_TYPES_C_H_
#include "../core.hpp"
#endif
