// gp_graph.hpp -- a caller-supplied graph (SRS v1-G) on the host:
// the admissibility check of a gp_graph and the transposed, deduplicated in-CSR the push-sum
// kernel walks.  Host-only: the standard library and the public header, nothing of HIP, so a host
// compiler can include it (tests/helpers/graph_check.cpp).  The LDS image the two CSRs take is
// gp_ensemble_shape.hpp's ens_graph_lds_bytes.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/gossip_hip.h"

namespace gp {

// The rules of an admissible graph, in the order they are tested for a node; 0: admissible.
enum GraphRule {
    GRAPH_OK = 0,
    GRAPH_NULL,       // a null pointer, a negative count or a non-zero reserved field
    GRAPH_POPULATION, // 2 <= P <= cap
    GRAPH_PTR_FIRST,  // indptr[0] = 0
    GRAPH_PTR_ORDER,  // indptr non-decreasing
    GRAPH_PTR_LAST,   // indptr[P] = E (no entry of indptr may exceed E)
    GRAPH_DEGREE,     // every node has an out-neighbour
    GRAPH_INDEX       // every index < P
};

// All or nothing: the first rule the lowest offending node breaks (nodes ascending; per node the
// rules in the order of GraphRule), with the text for gp_last_error() in `why`.  Reads indptr[i + 1]
// and the indices of node i only once everything below has passed, so no entry outside
// indptr[0..P] and indices[0..E) is touched whatever the arrays hold.
inline GraphRule graph_validate(const gp_graph* G, int64_t cap, std::string* why) {
    char buf[256];
    auto fail = [&](GraphRule r) {
        if (why) *why = buf;
        return r;
    };
    if (!G || !G->indptr || (!G->indices && G->num_edges != 0) || G->num_edges < 0 || G->reserved != 0) {
        snprintf(buf, sizeof buf, "graph: null graph, null indptr / indices, negative num_edges or reserved != 0");
        return fail(GRAPH_NULL);
    }
    const int64_t P = G->num_nodes, E = G->num_edges;
    if (P < 2 || P > cap) {
        snprintf(buf, sizeof buf, "graph: num_nodes %lld outside [2, %lld] (a graph needs an edge; the cap is one workgroup's node slots)",
                 (long long)P, (long long)cap);
        return fail(GRAPH_POPULATION);
    }
    if (G->indptr[0] != 0) {
        snprintf(buf, sizeof buf, "graph: node 0: indptr[0] must be 0 (got %lld)", (long long)G->indptr[0]);
        return fail(GRAPH_PTR_FIRST);
    }
    for (int64_t i = 0; i < P; ++i) {
        const int64_t b = G->indptr[i], e = G->indptr[i + 1];
        if (e < b) {
            snprintf(buf, sizeof buf, "graph: node %lld: indptr decreases (indptr[%lld] = %lld after %lld)", (long long)i,
                     (long long)(i + 1), (long long)e, (long long)b);
            return fail(GRAPH_PTR_ORDER);
        }
        if (e > E) {
            snprintf(buf, sizeof buf, "graph: node %lld: indptr[%lld] = %lld exceeds num_edges %lld (indptr[P] must be num_edges)",
                     (long long)i, (long long)(i + 1), (long long)e, (long long)E);
            return fail(GRAPH_PTR_LAST);
        }
        if (e == b) {
            snprintf(buf, sizeof buf, "graph: node %lld: degree 0 (every node needs an out-neighbour)", (long long)i);
            return fail(GRAPH_DEGREE);
        }
        for (int64_t q = b; q < e; ++q)
            if ((int64_t)G->indices[q] >= P) {
                snprintf(buf, sizeof buf, "graph: node %lld: neighbour index %u is not below num_nodes %lld", (long long)i,
                         (unsigned)G->indices[q], (long long)P);
                return fail(GRAPH_INDEX);
            }
    }
    if (G->indptr[P] != E) {
        snprintf(buf, sizeof buf, "graph: node %lld: indptr[P] = %lld must be num_edges %lld", (long long)(P - 1),
                 (long long)G->indptr[P], (long long)E);
        return fail(GRAPH_PTR_LAST);
    }
    return GRAPH_OK;
}

// Entries of the transposed graph with duplicates removed: distinct (sender, receiver) pairs.
// O(P) memory whatever E is, so the size of an image can be told before anything is allocated.
// The graph has passed graph_validate.
inline int64_t graph_in_entries(const gp_graph* G) {
    const int64_t P = G->num_nodes;
    std::vector<int64_t> last((size_t)P, -1);  // the highest sender seen for a receiver so far
    int64_t n = 0;
    for (int64_t i = 0; i < P; ++i)
        for (int64_t q = G->indptr[i]; q < G->indptr[i + 1]; ++q) {
            const uint32_t t = G->indices[q];
            if (last[t] != i) {
                last[t] = i;
                n += 1;
            }
        }
    return n;
}

// The two CSRs as the kernels stage them: 32-bit offsets, 16-bit ids (P <= 8192 < 0xFFFF).
struct GraphCsr {
    std::vector<uint32_t> out_off, in_off;  // P + 1 each
    std::vector<uint16_t> out_nbr, in_nbr;  // E_out (the caller's order), E_in
};

// out: the caller's lists as they are.  in: in_nbr[in_off[j] .. in_off[j + 1]) = the nodes that
// list j, ascending, each once -- a counting sort by receiver: the senders are visited in
// ascending order, so every receiver's run fills in ascending order, and a sender that lists a
// receiver twice is recognised by being the last one written there.  The graph has passed
// graph_validate and its entry counts fit 32 bits (the LDS check has run).
inline void graph_build(const gp_graph* G, GraphCsr* c) {
    const size_t P = (size_t)G->num_nodes, E = (size_t)G->num_edges;
    c->out_off.resize(P + 1);
    c->out_nbr.resize(E);
    for (size_t i = 0; i <= P; ++i) c->out_off[i] = (uint32_t)G->indptr[i];
    for (size_t q = 0; q < E; ++q) c->out_nbr[q] = (uint16_t)G->indices[q];
    std::vector<int64_t> last(P, -1);
    c->in_off.assign(P + 1, 0);
    for (size_t i = 0; i < P; ++i)
        for (uint32_t q = c->out_off[i]; q < c->out_off[i + 1]; ++q) {
            const uint16_t t = c->out_nbr[q];
            if (last[t] != (int64_t)i) {
                last[t] = (int64_t)i;
                c->in_off[t + 1] += 1;
            }
        }
    for (size_t j = 0; j < P; ++j) c->in_off[j + 1] += c->in_off[j];
    c->in_nbr.resize(c->in_off[P]);
    std::vector<uint32_t> fill(c->in_off.begin(), c->in_off.end() - 1);
    last.assign(P, -1);
    for (size_t i = 0; i < P; ++i)
        for (uint32_t q = c->out_off[i]; q < c->out_off[i + 1]; ++q) {
            const uint16_t t = c->out_nbr[q];
            if (last[t] != (int64_t)i) {
                last[t] = (int64_t)i;
                c->in_nbr[fill[t]++] = (uint16_t)i;
            }
        }
}

}  // namespace gp
