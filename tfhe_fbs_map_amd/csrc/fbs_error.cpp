// The error text of libfbsexec's calls (fbs_last_error): host code with no device in it, linked by the sanitizer harness of
// tests/c/ as well.
#include "fbs_internal.hpp"

namespace fbs {

static thread_local std::string g_create_error;

int set_error(const fbs_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}
const char *create_error() { return g_create_error.c_str(); }

}  // namespace fbs
