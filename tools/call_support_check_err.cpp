// call_support_check_err.cpp -- what tools/call_support_check.c needs of libgroot_host.so beside report.cpp: the last-error text
// (index.cpp has the library's own; linking that file would pull the whole index builder into a check of one function)
#include <cstdarg>
#include <cstdio>

#include "groot_host.h"

namespace groot {
static thread_local char g_err[1024];
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
} // namespace groot

extern "C" const char *groot_host_last_error(void) { return groot::g_err; }
