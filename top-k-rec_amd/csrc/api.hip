// Library-level entry points of libtkr_hip.so.
#include "tkr_common.h"
#include "../../include/tkr.h"

extern "C" int tkr_version(void) { return TKR_VERSION; }

// 0: the lab build that held the kernel forms measured and dropped is removed (include/tkr.h)
extern "C" int tkr_lab_build(void) { return 0; }
