// local_group.h -- the in-process transport's group, for 2D grids (misor_grid)
// and 3D grids (misor_grid3) alike: every rank of the group is a grid owned by
// its own host thread of ONE process (any devices, including all on one GPU).
// Collectives are a host barrier plus device-to-device copies; sums are
// combined in rank order.  It exists so the decomposed kernels can be run and
// checked on a single-GPU machine; across GPUs the RCCL path is used.
#pragma once

#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "misor.h"

template <class Grid>
struct LocalGroup {
    int n = 0;
    std::vector<Grid*> members;
    std::vector<double> vals;  // host scratch of an all-reduce, sized by the first to join
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0, joined = 0;
    long long generation = 0;

    void barrier() {
        std::unique_lock<std::mutex> lk(m);
        const long long gen = generation;
        if (++arrived == n) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return generation != gen; });
        }
    }
};

enum class LocalJoin { kNotLocal, kJoined, kBadMember };

// A comm_id that starts with "LOCAL:" names an in-process group: `grid` joins
// it as `rank` of `nranks` (the first to join creates it, with nvals doubles
// of scratch) and `name` receives its name.  kBadMember: the group has another
// size or the rank is taken.  Groups of each grid type have a registry of
// their own, and a name is free again once its last member has joined.
template <class Grid>
__attribute__((visibility("hidden")))  // with its registry: not exported from libmisor.so
LocalJoin join_local_group(const void* comm_id, int nranks, int rank, Grid* grid, size_t nvals,
                           std::shared_ptr<LocalGroup<Grid>>& out,
                           char (&name)[MISOR_COMM_ID_BYTES + 1]) {
    static constexpr char kLocalPrefix[] = "LOCAL:";
    static std::mutex mu;
    static std::map<std::string, std::shared_ptr<LocalGroup<Grid>>> groups;
    if (memcmp(comm_id, kLocalPrefix, sizeof kLocalPrefix - 1) != 0) return LocalJoin::kNotLocal;
    memcpy(name, comm_id, MISOR_COMM_ID_BYTES);
    name[MISOR_COMM_ID_BYTES] = '\0';
    std::lock_guard<std::mutex> lk(mu);
    auto& G = groups[name];
    if (!G) {
        G = std::make_shared<LocalGroup<Grid>>();
        G->n = nranks;
        G->members.assign(nranks, nullptr);
        G->vals.assign(nvals, 0.0);
    }
    if (G->n != nranks || G->members[rank]) return LocalJoin::kBadMember;
    G->members[rank] = grid;
    out = G;
    if (++G->joined == nranks) groups.erase(name);  // name reusable
    return LocalJoin::kJoined;
}
