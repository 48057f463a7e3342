// tests/tree_nodes_host.cpp — compiled by tests/test_tree_nodes_gpu.py WITHOUT the reference's headers and with
// -DNBODY_TREE=1 -DNBODY_TREE_NODES=1: the adaptor's Simulation() (the reference's 25 000 default bodies) steps once and the program
// walks `quadtree.nodes` the way the reference's drawQuadtreeNode does (main.cpp:394-475): a stack from the root, the four children
// of a branch at nodes[children + i], guarded by children + i < nodes.size().  Prints what it met.
#include <atomic>
#include <cstdio>
#include <vector>

#include "Simulation.hpp"

std::atomic<float> SIMULATION_DT{0.01f};

int main()
{
    try {
        Simulation sim;
        sim.step();
        const std::vector<Node> &nodes = sim.quadtree.nodes;
        size_t visited = 0, leaves = 0, branches = 0, deepest = 0;
        std::vector<size_t> stack;
        if (!nodes.empty()) stack.push_back(0);
        while (!stack.empty()) {
            const size_t i = stack.back();
            stack.pop_back();
            const Node &n = nodes[i];
            ++visited;
            if (n.depth > deepest) deepest = n.depth;
            if (n.is_branch()) {
                ++branches;
                for (size_t q = 0; q < 4; ++q)
                    if (n.children + q < nodes.size()) stack.push_back(n.children + q);
            } else if (!n.is_empty()) {
                ++leaves;
            }
        }
        printf("frame=%zu nodes=%zu visited=%zu leaves=%zu branches=%zu deepest=%zu\n", sim.frame, nodes.size(), visited, leaves, branches,
               deepest);
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
