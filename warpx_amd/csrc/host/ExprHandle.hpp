// What the C ABI's opaque `wxa_expr` is: a compiled wxa::host::Parser program plus, once a device entry has used it,
// its copy in device memory.  Plain C++ so that the host layer can wrap a Parser it already holds (a deck's
// density_function, a predefined profile built op by op) without going through a text again.
#ifndef WXA_HOST_EXPR_HANDLE_HPP_
#define WXA_HOST_EXPR_HANDLE_HPP_

#include <atomic>
#include <cstdint>

#include "Parser.hpp"

struct wxa_expr {
    wxa::host::Parser parser;
    uint64_t id = 0;                      // never reused: a workspace knows by it which programs it has uploaded
    // The program in device memory for wxa_expr_eval_device, owned.  That entry has no workspace whose DevBuf could hold
    // it, and this header is also compiled where there is no device runtime (the CPU build of the host layer): hence a
    // pointer with the deleter of whoever allocated it, not a DevBuf.  The injector's programs live in the workspace.
    void* dev = nullptr;
    void (*dev_free)(void*) = nullptr;

    explicit wxa_expr(const wxa::host::Parser& p) : parser(p) {
        static std::atomic<uint64_t> next{1};
        id = next.fetch_add(1);
    }
    wxa_expr(const wxa_expr&) = delete;
    wxa_expr& operator=(const wxa_expr&) = delete;
    ~wxa_expr() { if (dev && dev_free) dev_free(dev); }
};

#endif
