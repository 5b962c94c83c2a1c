// nrc_fail.hpp -- the library's error convention, for host code with and without a device (nrc_common.hpp includes it).
#pragma once
#include <stdexcept>
#include <string>

namespace nrc {

// Reference error convention: Log::Error(msg, true) throws std::runtime_error("SkyRenderer ERROR: " + msg)
// (src/Log.cpp:16-20); ASSERT_CUDA does the same (include/engine/cuda_common.hpp:14).
[[noreturn]] inline void fail(const std::string& msg) { throw std::runtime_error("SkyRenderer ERROR: " + msg); }

}  // namespace nrc
