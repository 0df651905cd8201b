// graph_check.cpp -- gp_graph.hpp on the host: the admissibility check and the transposed,
// deduplicated in-CSR (SRS v1-G), on a star, a directed cycle and a graph with
// self-loops and duplicate edges.  Stand-alone, built by tests/test_graph_host.py with the host
// compiler (with -fsanitize=address,undefined where those link).  Prints one line per check and
// "graph_check ok <n>" at the end; exits 1 on the first failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../gossipprotocol_amd/csrc/gp_graph.hpp"

static int checks = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checks;                                                     \
        if (!(cond)) {                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
            exit(1);                                                  \
        }                                                             \
    } while (0)

using gp::GraphCsr;
using Lists = std::vector<std::vector<uint32_t>>;

struct Owned {  // exact-size heap arrays, so a read past either end is the sanitizer's to see
    std::vector<int64_t> indptr;
    std::vector<uint32_t> indices;
    gp_graph g{};
    explicit Owned(const Lists& l) {
        indptr.push_back(0);
        for (const auto& a : l) {
            indices.insert(indices.end(), a.begin(), a.end());
            indptr.push_back((int64_t)indices.size());
        }
        indices.shrink_to_fit();
        indptr.shrink_to_fit();
        sync();
        g.num_nodes = (int64_t)l.size();
        g.num_edges = (int64_t)indices.size();
    }
    void sync() {
        g.indptr = indptr.data();
        g.indices = indices.data();
    }
};

static Lists in_of(const GraphCsr& c, size_t P) {
    Lists r(P);
    for (size_t j = 0; j < P; ++j) r[j].assign(c.in_nbr.begin() + c.in_off[j], c.in_nbr.begin() + c.in_off[j + 1]);
    return r;
}

static void transpose_is(const Lists& out, const Lists& want_in, const char* what) {
    Owned o(out);
    std::string why;
    CHECK(gp::graph_validate(&o.g, 8192, &why) == gp::GRAPH_OK);
    size_t e_in = 0;
    for (const auto& a : want_in) e_in += a.size();
    CHECK(gp::graph_in_entries(&o.g) == (int64_t)e_in);
    GraphCsr c;
    gp::graph_build(&o.g, &c);
    const size_t P = out.size();
    CHECK(c.out_off.size() == P + 1 && c.in_off.size() == P + 1);
    CHECK(c.out_nbr.size() == o.indices.size() && c.in_nbr.size() == e_in);
    CHECK(c.out_off[0] == 0 && c.in_off[0] == 0 && c.out_off[P] == o.indices.size() && c.in_off[P] == e_in);
    for (size_t q = 0; q < o.indices.size(); ++q) CHECK(c.out_nbr[q] == o.indices[q]);  // the caller's order
    CHECK(in_of(c, P) == want_in);
    for (size_t j = 0; j < P; ++j)  // ascending and deduplicated
        for (uint32_t e = c.in_off[j] + 1; e < c.in_off[j + 1]; ++e) CHECK(c.in_nbr[e - 1] < c.in_nbr[e]);
    printf("transpose %s: %zu out, %zu in\n", what, o.indices.size(), e_in);
}

static void refused(Owned& o, gp::GraphRule rule, const char* words, int64_t cap = 8192) {
    o.sync();
    std::string why;
    const gp::GraphRule got = gp::graph_validate(&o.g, cap, &why);
    printf("refused (%d): %s\n", (int)got, why.c_str());
    CHECK(got == rule);
    CHECK(strstr(why.c_str(), words) != nullptr);
}

int main() {
    // a star of 65: the hub's in-list is every leaf, each leaf's is the hub
    {
        Lists out(65), in(65);
        for (uint32_t i = 1; i < 65; ++i) {
            out[0].push_back(i);
            out[i].push_back(0);
            in[0].push_back(i);
            in[i].push_back(0);
        }
        transpose_is(out, in, "star(65)");
    }
    // a directed cycle of 40: i lists i + 1, so the in-list of j is j - 1 -- not its out-list
    {
        Lists out(40), in(40);
        for (uint32_t i = 0; i < 40; ++i) {
            out[i].push_back((i + 1) % 40);
            in[(i + 1) % 40].push_back(i);
        }
        transpose_is(out, in, "cycle(40)");
    }
    // self-loops and duplicates, lists in no particular order
    transpose_is({{3, 0, 3, 1}, {1, 1}, {0, 3, 0}, {2}}, {{0, 2}, {0, 1}, {3}, {0, 2}}, "loops and duplicates");
    // the largest population: ids up to 8191 survive the 16-bit entries
    {
        Lists out(8192), in(8192);
        for (uint32_t i = 0; i < 8192; ++i) {
            out[i].push_back(8191 - i);
            in[8191 - i].push_back(i);
        }
        transpose_is(out, in, "reversal(8192)");
    }

    const Lists ok = {{1, 2}, {2}, {0, 1}};
    {
        Owned o(ok);
        o.indptr[0] = 1;
        refused(o, gp::GRAPH_PTR_FIRST, "node 0: indptr[0] must be 0");
    }
    {
        Owned o(ok);
        o.indptr[2] = 1;  // 0 2 1 5: node 1 ends before it starts
        refused(o, gp::GRAPH_PTR_ORDER, "node 1: indptr decreases");
    }
    {
        Owned o(ok);
        o.indptr[3] = 7;  // past the indices: must be refused without reading them
        refused(o, gp::GRAPH_PTR_LAST, "node 2: indptr[3] = 7 exceeds num_edges 5");
    }
    {
        Owned o(ok);
        o.indptr[3] = 4;
        refused(o, gp::GRAPH_PTR_LAST, "node 2: indptr[P] = 4 must be num_edges 5");
    }
    {
        Owned o(ok);
        o.indptr[2] = 2;  // 0 2 2 5
        refused(o, gp::GRAPH_DEGREE, "node 1: degree 0");
    }
    {
        Owned o(ok);
        o.indices[2] = 3;
        refused(o, gp::GRAPH_INDEX, "node 1: neighbour index 3 is not below num_nodes 3");
    }
    {
        Owned o(ok);  // two offenders: the lowest node is named, and its first rule
        o.indices[0] = 9;
        o.indptr[2] = 2;
        refused(o, gp::GRAPH_INDEX, "node 0: neighbour index 9");
    }
    {
        const Lists one = {{0}};
        Owned o(one);
        refused(o, gp::GRAPH_POPULATION, "num_nodes 1 outside [2, 8192]");
    }
    {
        Owned o(ok);
        refused(o, gp::GRAPH_POPULATION, "num_nodes 3 outside [2, 2]", 2);
    }
    {
        Owned o(ok);
        o.g.reserved = 1;
        refused(o, gp::GRAPH_NULL, "reserved");
        o.g.reserved = 0;
        o.sync();
        o.g.indptr = nullptr;
        std::string why;
        CHECK(gp::graph_validate(&o.g, 8192, &why) == gp::GRAPH_NULL);
        CHECK(gp::graph_validate(nullptr, 8192, &why) == gp::GRAPH_NULL);
    }
    printf("graph_check ok %d\n", checks);
    return 0;
}
