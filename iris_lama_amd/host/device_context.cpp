// device_context.cpp -- lama::DeviceContext (include/lama/device_context.h) and the text of a refused device call.
#include "lama/device_context.h"

#include <stdexcept>

#include "hip_engine.hpp"

namespace lama {

const char* lastDeviceError(const HipEngine& e, const lama_hip_ctx* ctx)
{
    const char* msg = e.last_error ? e.last_error(ctx) : "";
    return msg ? msg : "";
}

std::string deviceFailure(const HipEngine& e, const lama_hip_ctx* ctx, const char* who, const char* what, int32_t rc)
{
    return std::string(who) + ": " + what + " failed (status " + std::to_string(rc) + "): " + lastDeviceError(e, ctx);
}

void DeviceContext::create(std::shared_ptr<HipEngine> engine, const lama_hip_cfg& cfg)
{
    reset();
    eng_ = std::move(engine);
    const int32_t rc = eng_->ctx_create(&cfg, &ctx_);
    if (rc != 0 || !ctx_) {
        ctx_ = nullptr;
        throw std::runtime_error(std::string(owner_) + ": lama_hip_ctx_create failed (status " + std::to_string(rc) +
                                 "): no usable MI355X / HIP device; there is no CPU fallback");
    }
}

void DeviceContext::reset()
{
    if (ctx_) eng_->ctx_destroy(ctx_);
    ctx_ = nullptr;
}

void DeviceContext::check(int32_t rc, const char* what) const
{
    if (rc) throw std::runtime_error(deviceFailure(*eng_, ctx_, owner_, what, rc));
}

bool DeviceContext::download(uint32_t particle, int32_t kind, std::vector<uint64_t>& ids, std::vector<uint8_t>& cells, std::vector<uint64_t>& masks) const
{
    uint32_t n = 0, got = 0;
    if (!ctx_ || eng_->pf_map_patches(ctx_, particle, kind, &n) != 0) return false;
    ids.assign(n, 0);
    cells.assign((size_t)n * kCellsPerPatch * (kind == LAMA_HIP_MAP_DISTANCE ? kDistanceCellBytes : kOccupancyCellBytes), 0);
    masks.assign((size_t)n * kMaskWordsPerPatch, 0);
    if (n == 0) return true;
    return eng_->pf_download_map(ctx_, particle, kind, n, ids.data(), cells.data(), masks.data(), &got) == 0 && got == n;
}

} // namespace lama
