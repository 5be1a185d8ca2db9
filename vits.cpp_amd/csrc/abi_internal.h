// abi_internal.h — what the operator-level files (abi_ops_*.cpp) share with abi.cpp: the one thread-local error string behind vits_last_error() and the
// try / catch frame of every entry point. Nothing here is exported.
#pragma once
#include <exception>
#include <string>

namespace vits {
void set_err(const std::string& e);  // abi.cpp: sets what vits_last_error() returns on this thread
inline int fail(const char* what) {
    set_err(what);
    return -1;
}
inline int fail(const std::string& what) { return fail(what.c_str()); }
}  // namespace vits
using vits::fail;
using vits::set_err;

#define VITS_TRY try {
#define VITS_CATCH(ret)                           \
    }                                             \
    catch (const std::exception& e) {             \
        set_err(e.what());                        \
        return ret;                               \
    }                                             \
    catch (...) {                                 \
        set_err("unknown exception");             \
        return ret;                               \
    }
