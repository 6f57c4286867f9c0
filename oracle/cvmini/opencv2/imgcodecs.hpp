/* cvmini: forwards to opencv2/core.hpp, the one real stand-in header. */
#ifndef CVMINI_OPENCV2_IMGCODECS_HPP_
#define CVMINI_OPENCV2_IMGCODECS_HPP_
#include "core.hpp"
#endif
