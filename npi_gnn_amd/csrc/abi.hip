// What every entry point of include/npi_gnn.h shares: the thread's last error text and the ABI version.  No kernel.
#include "npi_common.h"
#include <stdarg.h>

namespace npi {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace npi

extern "C" const char* npi_last_error(void) { return npi::g_err; }
extern "C" int npi_abi_version(void) { return 4; }
