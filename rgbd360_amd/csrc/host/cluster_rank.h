// cluster_rank.h — the host side of the cluster ranking (host only, no HIP): the components within the size bounds, as
// (root, size) records in any order, into rank order (size descending, ties by root ascending) with the tables the
// device reads back.  DESIGN.md §5b-4; tests/host/cluster_host_check.cpp runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <algorithm>
#include <vector>

struct ClusterRankRec { int root, size; };

// rank_root [nk]: the roots in rank order; off [nk + 1]: the first member of every cluster in the rank-ordered member
// list; cpre [nk + 1]: the first chunk of `chunk` members of every cluster.  Returns the number of members.
inline size_t cluster_rank_tables(const ClusterRankRec* rec, size_t nk, unsigned chunk, std::vector<int>& rank_root,
                                  std::vector<unsigned>& off, std::vector<unsigned>& cpre) {
    std::vector<ClusterRankRec> v(rec, rec + nk);
    std::sort(v.begin(), v.end(), [](const ClusterRankRec& a, const ClusterRankRec& b) {
        return a.size != b.size ? a.size > b.size : a.root < b.root;
    });
    rank_root.resize(nk);
    off.assign(nk + 1, 0u);
    cpre.assign(nk + 1, 0u);
    for (size_t r = 0; r < nk; ++r) {
        rank_root[r] = v[r].root;
        off[r + 1] = off[r] + (unsigned)v[r].size;
        cpre[r + 1] = cpre[r] + ((unsigned)v[r].size + chunk - 1) / chunk;
    }
    return off[nk];
}
