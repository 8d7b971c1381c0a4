// Handle types behind the C ABI (include/policygpu.h) and what every capi_*.cpp needs around a
// call on a pg_ctx: fail, DEVICE_GUARD, GUARD_BEGIN / GUARD_END, host_view.
#pragma once
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "../../include/policygpu.h"
#include "configurator.hpp"
#include "engine.hpp"

struct pg_ctx {
    pg::Engine eng;
};
struct pg_renderer {
    pg_ctx* ctx;
    std::unique_ptr<pg::Renderer> r;
};
struct pg_txn {
    pg_ctx* ctx;
    std::unique_ptr<pg::RendererTxn> t;
};
struct pg_mock_renderer {
    pg::MockRenderer r;
};
struct pg_configurator {
    pg::PolicyConfigurator c;
    std::vector<std::unique_ptr<pg::CfgRenderer>> adapters;  // GPU renderers seen as configurator sinks
    std::string last_error;
};
struct pg_cfg_txn {
    pg_configurator* c;
    std::unique_ptr<pg::PolicyConfiguratorTxn> t;
};

namespace pg {
// pg_ipnet <-> net.IPNet (IPv4: 4-byte address and mask, as net.ParseCIDR returns them)
IPNet to_ipnet(const pg_ipnet& n);
pg_ipnet to_pg_ipnet(const IPNet& n);
// host view of the compiled table set (pointers into the host image; capi.cpp)
DevTableSet host_view(const HostTableSet& h);

inline int fail(pg_ctx* c, int code, const std::string& msg) {
    if (c) c->eng.last_error = msg;
    return code;
}

// Every entry point that touches the device makes the context's GPU current for the call and
// restores the caller's afterwards: contexts on different GPUs can share a process, and a cgo
// caller's goroutine may move between OS threads between two calls.
struct DeviceGuard {
    int prev = -1, dev = 0;
    bool ok = true;
    std::string err;
    explicit DeviceGuard(const pg_ctx* c) : dev(c->eng.device) {
        if (dev_get_device(&prev) != 0) prev = -1;
        if (prev != dev) ok = dev_set_device(dev, &err) == 0;
    }
    ~DeviceGuard() {
        if (prev >= 0 && prev != dev) (void)dev_set_device(prev, nullptr);
    }
};
}  // namespace pg

#define DEVICE_GUARD(ctx)                                             \
    pg::DeviceGuard guard_(ctx);                                      \
    if (!guard_.ok) return pg::fail(ctx, PG_EIO, "set device: " + guard_.err)

#define GUARD_BEGIN try {
#define GUARD_END(ctx)                                             \
    }                                                              \
    catch (const std::exception& e) {                              \
        return pg::fail(ctx, PG_EFAULT, e.what());                 \
    }                                                              \
    catch (...) {                                                  \
        return pg::fail(ctx, PG_EFAULT, "unknown C++ exception");  \
    }
