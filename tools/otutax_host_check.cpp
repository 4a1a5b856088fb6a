// A stand-alone check of the host side of the consensus taxonomy of the OTUs (raxtax_amd/csrc/host_otutax.cpp: rtx_otu_taxonomy_host, its view
// and formatter, rtx_result_best_lineages) for the sanitizers: the member lists are built by a counting sort, the paths are walked over index
// arrays and the records are cut out of rows of exactly their lengths, so they are built with -fsanitize=address,undefined together with this
// main.  Build and run, on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Iraxtax_amd/csrc tools/otutax_host_check.cpp \
//       raxtax_amd/csrc/host_otutax.cpp raxtax_amd/csrc/host_tally.cpp -o otutax_host_check && ./otutax_host_check
// The tree is made by hand (no parser, no k-mer map): the two functions read its lineages and its flat nodes alone.  The result is held
// against a restatement written here: per OTU and node the clade by a scan over all rows.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "raxtax_hip.h"
#include "rtx_internal.hpp"

namespace rtx {
void set_error(const char *, ...) {}  // (the library's lives in rtx_api_index.hip)
unsigned host_threads(unsigned, unsigned) { return 1; }
}  // namespace rtx

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "otutax_host_check: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// a tree of fan-out 3, 3, 2 with one chain of RTX_MAX_DEPTH levels beside it: breadth first, one lineage per leaf
static void make_tree(rtx_tree &t) {
    rtx::FlatNodes &f = t.flat;
    struct N { uint32_t parent, depth; std::string name; };
    std::vector<N> all{{rtx::kNoNode, 0, ""}};
    std::vector<uint32_t> level{0};
    const uint32_t fan[3] = {3, 3, 2};
    for (uint32_t d = 0; d < 3; d++) {
        std::vector<uint32_t> next;
        for (uint32_t v : level)
            for (uint32_t c = 0; c < fan[d]; c++) {
                next.push_back((uint32_t)all.size());
                all.push_back({v, d + 1, (all[v].name.empty() ? "" : all[v].name + ",") + "t" + std::to_string(d) + std::to_string(next.size())});
            }
        level = next;
    }
    uint32_t up = 0;
    std::string name;
    for (uint32_t d = 1; d <= RTX_MAX_DEPTH; d++) {  // the chain, appended; the sort below puts every node with its level
        name += (d > 1 ? ",c" : "c") + std::to_string(d - 1);
        all.push_back({up, d, name});
        up = (uint32_t)all.size() - 1;
    }
    // sort by depth, stable, and renumber the parents
    std::vector<uint32_t> order(all.size());
    for (uint32_t v = 0; v < all.size(); v++) order[v] = v;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return all[a].depth < all[b].depth; });
    std::vector<uint32_t> where(all.size());
    for (uint32_t i = 0; i < order.size(); i++) where[order[i]] = i;
    const uint32_t nn = (uint32_t)all.size();
    f.parent.assign(nn, rtx::kNoNode);
    f.depth.assign(nn, 0);
    f.begin.assign(nn, 0);
    f.end.assign(nn, 0);
    f.first_child.assign(nn, 0);
    f.n_children.assign(nn, 0);
    f.type.assign(nn, (uint8_t)rtx::kInner);
    std::vector<std::string> names(nn);
    for (uint32_t i = 0; i < nn; i++) {
        const N &n = all[order[i]];
        f.parent[i] = n.parent == rtx::kNoNode ? rtx::kNoNode : where[n.parent];
        f.depth[i] = n.depth;
        f.max_depth = std::max(f.max_depth, n.depth);
        names[i] = n.name;
    }
    // the lineages: the names of the leaves, sorted; a node's range is the lineages it is a prefix of
    std::vector<bool> leaf(nn, true);
    for (uint32_t i = 1; i < nn; i++) leaf[f.parent[i]] = false;
    for (uint32_t i = 1; i < nn; i++)
        if (leaf[i]) t.lineages.push_back(names[i]);
    std::sort(t.lineages.begin(), t.lineages.end());
    for (uint32_t i = 1; i < nn; i++) {
        uint32_t lo = (uint32_t)t.lineages.size(), hi = 0;
        for (uint32_t l = 0; l < t.lineages.size(); l++) {
            const std::string &s = t.lineages[l];
            if (s.compare(0, names[i].size(), names[i]) == 0 && (s.size() == names[i].size() || s[names[i].size()] == ',')) { lo = std::min(lo, l); hi = std::max(hi, l + 1); }
        }
        f.begin[i] = lo;
        f.end[i] = hi;
        if (leaf[i]) f.type[i] = (uint8_t)rtx::kTaxon;
    }
    f.end[0] = (uint32_t)t.lineages.size();
    t.n = t.num_tips = t.lineages.size();
}

int main() {
    rtx_tree tree;
    make_tree(tree);
    const rtx::FlatNodes &f = tree.flat;
    const uint32_t nn = f.size();
    CHECK(f.max_depth == RTX_MAX_DEPTH && nn == 1 + 4 + 9 + 18 + (RTX_MAX_DEPTH - 1));
    for (uint32_t v = 1; v < nn; v++) CHECK(f.parent[v] < v && f.depth[v] == f.depth[f.parent[v]] + 1 && f.begin[v] < f.end[v]);
    rtx_nodes_view nodes{};
    nodes.n_nodes = nn;
    nodes.node_parent = f.parent.data();

    // rows on random nodes, the arrays at their exact lengths (a read past an end is the sanitizer's)
    std::mt19937 rng(7);
    const uint64_t n_rows = 3000, n_otus = 200;
    const uint32_t stride = RTX_MAX_DEPTH;
    std::unique_ptr<uint32_t[]> otu(new uint32_t[n_rows]), node(new uint32_t[n_rows]), seed(new uint32_t[n_otus]);
    std::unique_ptr<uint64_t[]> weight(new uint64_t[n_rows]);
    std::unique_ptr<uint8_t[]> kind(new uint8_t[n_rows]), L(new uint8_t[n_rows]), hund(new uint8_t[n_rows * stride]);
    memset(hund.get(), 0, n_rows * stride);
    for (uint64_t r = 0; r < n_rows; r++) {
        otu[r] = r < n_otus ? (uint32_t)r : (uint32_t)(rng() % 8 ? rng() % 20 : rng() % n_otus);  // every OTU has a row; twenty of them are large
        weight[r] = 1 + rng() % 1000;
        const uint32_t v = rng() % 6 ? 1 + rng() % (nn - 1) : 0;
        node[r] = v;
        L[r] = (uint8_t)f.depth[v];
        kind[r] = v ? RTX_LIN_CLASSIFIED : (rng() % 2 ? RTX_LIN_UNCLASSIFIED : RTX_LIN_UNCLASSIFIABLE);
        for (uint32_t d = 0; d < L[r]; d++) hund[r * stride + d] = (uint8_t)(50 + rng() % 51);
    }
    for (uint64_t k = 0; k < n_otus; k++) seed[k] = (uint32_t)k;
    const rtx_lineage_records rec{kind.get(), L.get(), node.get(), hund.get(), stride};
    rtx_otutax *tax = nullptr;
    for (uint32_t pct : {50u, 101u}) {
        const rtx_otu_taxonomy_params bad{pct, 0};
        CHECK(rtx_otu_taxonomy_host(n_rows, otu.get(), weight.get(), n_otus, seed.get(), &rec, &nodes, &bad, &tax) == RTX_ERR_INVALID && tax == nullptr);
    }
    for (uint32_t pct : {51u, 67u, 100u}) {
        const rtx_otu_taxonomy_params prm{pct, 0};
        CHECK(rtx_otu_taxonomy_host(n_rows, otu.get(), weight.get(), n_otus, seed.get(), &rec, &nodes, &prm, &tax) == RTX_OK);
        rtx_otu_taxonomy_view_t v{};
        CHECK(rtx_otu_taxonomy_view(tax, &v) == RTX_OK && v.n_rows == n_rows && v.n_otus == n_otus && v.stride == RTX_MAX_DEPTH && v.agree_pct == pct);
        uint64_t walked = 0;
        for (uint64_t k = 0; k < n_otus; k++) {
            // the restatement: the clade of node x in OTU k is the weight of the members with x on the way from their node to the root
            auto clade = [&](uint32_t x, uint64_t *conf) {
                uint64_t c = 0;
                *conf = 0;
                for (uint64_t r = 0; r < n_rows; r++) {
                    if (otu[r] != k || L[r] == 0) continue;
                    for (uint32_t u = node[r]; u != 0; u = f.parent[u])
                        if (u == x) { c += weight[r]; *conf += weight[r] * hund[r * stride + f.depth[x] - 1]; }
                }
                return c;
            };
            uint64_t size = 0, members = 0, classified = 0;
            for (uint64_t r = 0; r < n_rows; r++)
                if (otu[r] == k) { size += weight[r]; members++; classified += kind[r] == RTX_LIN_CLASSIFIED ? weight[r] : 0; }
            CHECK(v.sizes[k] == size && v.members[k] == members && v.classified[k] == classified);
            uint32_t cur = 0, depth = 0;
            for (;;) {
                uint32_t next = 0, found = 0;
                uint64_t cl = 0, cf = 0;
                for (uint32_t x = 1; x < nn; x++) {
                    if (f.parent[x] != cur) continue;
                    uint64_t conf = 0;
                    const uint64_t c = clade(x, &conf);
                    if (c * 100 >= (uint64_t)pct * size) { next = x; cl = c; cf = conf; found++; }
                }
                CHECK(found <= 1);
                if (!found) break;
                CHECK(depth < v.stride && v.clade[k * v.stride + depth] == cl && v.conf[k * v.stride + depth] == cf);
                cur = next;
                depth++;
            }
            CHECK(v.depth[k] == depth && v.node[k] == cur && v.seed_rel[k] <= 3);
            for (uint32_t d = depth; d < v.stride; d++) CHECK(v.clade[k * v.stride + d] == 0 && v.conf[k * v.stride + d] == 0);
            walked += depth;
        }
        CHECK(pct == 100 || walked > 50);
        // the formatter into a buffer of exactly `need` bytes, and one byte less
        const int64_t need = rtx_otu_taxonomy_format(tax, &tree, 2, nullptr, 0);
        CHECK(need > 0);
        std::unique_ptr<char[]> buf(new char[(size_t)need]);
        CHECK(rtx_otu_taxonomy_format(tax, &tree, 2, buf.get(), (uint64_t)need) == need && buf[(size_t)need - 1] == '\n');
        CHECK(rtx_otu_taxonomy_format(tax, &tree, 2, buf.get(), (uint64_t)need - 1) == -need - (int64_t)RTX_NEED_BASE);
        double s[4];
        CHECK(rtx_otu_taxonomy_times(tax, s) == RTX_OK && s[0] == 0 && s[3] == 0);
        rtx_otu_taxonomy_destroy(tax);
        tax = nullptr;
    }
    // no rows at all
    CHECK(rtx_otu_taxonomy_host(0, nullptr, nullptr, 0, nullptr, &rec, &nodes, nullptr, &tax) == RTX_OK);
    CHECK(rtx_otu_taxonomy_format(tax, &tree, 0, nullptr, 0) > 0);
    rtx_otu_taxonomy_destroy(tax);

    // rtx_result_best_lineages over a hand-made view: rows of the tree's depth exactly (stride = the deepest lineage), both with the byte
    // arrays and without; every query with one row but the last two (no row; a status that is not RTX_Q_OK)
    const uint32_t nq = 64, D = f.max_depth;
    std::unique_ptr<uint32_t[]> t_(new uint32_t[nq]), count(new uint32_t[nq]), lin(new uint32_t[nq]), rnode(new uint32_t[nq]), rdepth(new uint32_t[nq]);
    std::unique_ptr<uint8_t[]> status(new uint8_t[nq]), depth8(new uint8_t[nq]), h8(new uint8_t[(size_t)nq * D]);
    std::unique_ptr<uint64_t[]> begin(new uint64_t[nq]);
    std::unique_ptr<double[]> gs(new double[nq]), conf(new double[(size_t)nq * D]), local(new double[nq]);
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t v = 1 + rng() % (nn - 1);
        t_[q] = 30; status[q] = q == nq - 1; count[q] = q == nq - 2 ? 0 : 1; begin[q] = nq - 1 - q;  // rows in another order than the queries
        const uint32_t r = nq - 1 - q;
        lin[r] = f.begin[v]; rnode[r] = v; rdepth[r] = f.depth[v]; depth8[r] = (uint8_t)f.depth[v]; gs[q] = 1.0; local[r] = 1.0;
        for (uint32_t d = 0; d < D; d++) {
            h8[(size_t)r * D + d] = d < f.depth[v] ? (uint8_t)(d < 2 ? 100 : 60 + rng() % 41) : 0;
            conf[(size_t)r * D + d] = h8[(size_t)r * D + d] / 100.0;
        }
    }
    std::unique_ptr<uint64_t[]> xoff(new uint64_t[nq + 1]);
    std::vector<uint32_t> xids;
    xoff[0] = 0;
    for (uint32_t q = 0; q < nq; q++) {  // no, one or two exact matches
        for (uint32_t i = 0; i < q % 3; i++) xids.push_back(rng() % (uint32_t)tree.lineages.size());
        xoff[q + 1] = xids.size();
    }
    std::unique_ptr<uint32_t[]> ids(new uint32_t[xids.size()]);
    memcpy(ids.get(), xids.data(), xids.size() * 4);
    for (int bytes = 0; bytes < 2; bytes++) {
        rtx_result_view res{};
        res.n_queries = nq; res.n_rows = nq; res.t = t_.get(); res.status = status.get(); res.global_signal = gs.get(); res.row_begin = begin.get(); res.row_count = count.get();
        res.row_lineage = lin.get(); res.row_node = rnode.get(); res.row_depth = rdepth.get(); res.row_conf = conf.get(); res.row_local_signal = local.get();
        res.row_conf_stride = D;
        if (bytes) { res.row_depth_u8 = depth8.get(); res.row_conf_hundredths = h8.get(); }
        for (uint32_t flags : {0u, (uint32_t)RTX_SKIP_EXACT_MATCHES, (uint32_t)RTX_RAW_CONFIDENCE}) {
            std::unique_ptr<uint8_t[]> k2(new uint8_t[nq]), l2(new uint8_t[nq]), h2(new uint8_t[(size_t)nq * D]);
            std::unique_ptr<uint32_t[]> n2(new uint32_t[nq]);
            CHECK(rtx_result_best_lineages(&tree, &res, ids.get(), xoff.get(), 80, flags, k2.get(), l2.get(), n2.get(), h2.get(), D) == RTX_OK);
            for (uint32_t q = 0; q < nq; q++) {
                if (q >= nq - 2) { CHECK(k2[q] == RTX_LIN_UNCLASSIFIABLE && l2[q] == 0); continue; }
                const uint32_t r = nq - 1 - q;
                if (flags == 0 && q % 3 == 1) {  // the override: the reference's own leaf, 100 on every level
                    const std::string &s = tree.lineages[ids[xoff[q]]];
                    const uint32_t levels = 1 + (uint32_t)std::count(s.begin(), s.end(), ',');
                    CHECK(k2[q] == RTX_LIN_CLASSIFIED && l2[q] == levels && f.depth[n2[q]] == levels && f.begin[n2[q]] == ids[xoff[q]] && h2[(size_t)q * D + levels - 1] == 100);
                    continue;
                }
                uint32_t want = 0;
                while (want < rdepth[r] && h8[(size_t)r * D + want] >= 80) want++;
                CHECK(l2[q] == want && k2[q] == (want ? RTX_LIN_CLASSIFIED : RTX_LIN_UNCLASSIFIED) && want >= 1);
                uint32_t u = rnode[r];
                for (uint32_t d = rdepth[r]; d > want; d--) u = f.parent[u];
                CHECK(n2[q] == u);
                for (uint32_t d = 0; d < D; d++) CHECK(h2[(size_t)q * D + d] == (d < want ? h8[(size_t)r * D + d] : 0));
            }
        }
        std::unique_ptr<uint8_t[]> k2(new uint8_t[nq]), l2(new uint8_t[nq]), h2(new uint8_t[(size_t)nq * D]);
        std::unique_ptr<uint32_t[]> n2(new uint32_t[nq]);
        CHECK(rtx_result_best_lineages(&tree, &res, nullptr, nullptr, 0, 0, k2.get(), l2.get(), n2.get(), h2.get(), D) == RTX_ERR_INVALID);
        CHECK(rtx_result_best_lineages(&tree, &res, nullptr, nullptr, 80, 0, k2.get(), l2.get(), n2.get(), h2.get(), D - 1) == RTX_ERR_INVALID);
    }
    printf("otutax_host_check: ok (%u nodes, %llu rows, %llu OTUs)\n", nn, (unsigned long long)n_rows, (unsigned long long)n_otus);
    return 0;
}
