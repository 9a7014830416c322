/* crtdbg.h -- stand-in for MSVC's debug-heap header; see prelude.h. */
#pragma once
#include <cassert>
#ifndef _ASSERT
#define _ASSERT(x) assert(x)
#define _ASSERTE(x) assert(x)
#endif
