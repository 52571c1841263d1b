// rp_host_util.h -- what librp_host.so's translation units share: the thread's last error (rph_last_error).  Internal.
#pragma once
#include <string>

#include "../../include/rp_host.h"

namespace rph {

// The calling thread's last error becomes m; returns code (RP_EINVAL: what nearly every refusal is).
int fail(int code, const std::string& m);
inline int fail(const std::string& m) { return fail(RP_EINVAL, m); }

}  // namespace rph
