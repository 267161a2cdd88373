#include "rt_common.h"
#define RT_STR_(x) #x
#define RT_STR(x) RT_STR_(x)
extern "C" const char* rt_version(void) { return "reptext_hip abi" RT_STR(RT_ABI_VERSION) " gfx950"; }
extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }
