// sc_diag_blob.h -- how the host-plan diag entries (sc_diag_ivf_plan, sc_diag_encoder_plan) hand a set of named arrays to their caller:
// records of {char name[16]; int32 kind (0 i32, 1 i64, 2 u32, 3 IvfCoarseItem); int32 0; int64 count; data padded to 8 bytes}
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

struct DiagBlob {
    std::vector<char> bytes;
    void put(const char* name, int kind, const void* data, size_t count, size_t elem) {
        char head[32] = {0};
        strncpy(head, name, 15);
        const int32_t kd = kind;
        const int64_t n = (int64_t)count;
        memcpy(head + 16, &kd, 4);
        memcpy(head + 24, &n, 8);
        bytes.insert(bytes.end(), head, head + 32);
        if (count) bytes.insert(bytes.end(), (const char*)data, (const char*)data + count * elem);
        bytes.resize((bytes.size() + 7) & ~(size_t)7, 0);
    }
    void i32(const char* name, const std::vector<int32_t>& v) { put(name, 0, v.data(), v.size(), 4); }
    void i64(const char* name, const std::vector<int64_t>& v) { put(name, 1, v.data(), v.size(), 8); }
    void num(const char* name, int64_t v) { put(name, 1, &v, 1, 8); }
    // *need_bytes = the total size; the records go to `out` when cap_bytes holds them
    void give(void* out, int64_t cap_bytes, int64_t* need_bytes) const {
        *need_bytes = (int64_t)bytes.size();
        if (out && cap_bytes >= *need_bytes) memcpy(out, bytes.data(), bytes.size());
    }
};
