// rescued_bam_check_stubs.cpp -- what tools/rescued_bam_check.c needs of libgroot_host.so beside bam.cpp: the last-error text, the
// version string of the header and the thread count (index.cpp has the library's own; linking that file would pull the whole index
// builder into a check of one function)
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
unsigned usable_cpus() { return 1; }
} // namespace groot

extern "C" const char *groot_host_last_error(void) { return groot::g_err; }
extern "C" const char *groot_host_version(void) { return "1.1.2"; }
