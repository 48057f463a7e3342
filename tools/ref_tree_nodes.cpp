// tools/ref_tree_nodes.cpp — FIXTURE GENERATOR ONLY (never linked into the product, never built by the package).
//
// Records what the compiled reference's Quadtree::build leaves in `quadtree.nodes` and the layout of its `Node`.  The reference's
// headers are included BY PATH (-I<reference>/Nbodysim/headers), unmodified, like oracle/ref_harness.cpp does; nothing of them is
// copied.  Driven by tools/make_tree_nodes_golden.py, which states the compiler command.
//
//   ref_tree_nodes --layout              JSON on stdout: sizeof, alignof and the nine field offsets of Node
//   ref_tree_nodes IN.bin OUT.bin        IN: n x {x, y, mass} float32; OUT: one packed 48-byte row per node of quadtree.nodes after
//                                        Quadtree::build: pos.x, pos.y, mass, center.x, center.y, size (float32), children, next,
//                                        depth (uint64)
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "Body.hpp"
#include "Quadtree.hpp"

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "--layout")) {
        using Data = decltype(Node::data);
        const size_t data = offsetof(Node, data);
        printf("{\n \"sizeof_Node\": %zu,\n \"alignof_Node\": %zu,\n \"off_data_pos\": %zu,\n \"off_data_mass\": %zu,\n"
               " \"off_data_quad_center\": %zu,\n \"off_data_quad_size\": %zu,\n \"off_children\": %zu,\n \"off_next\": %zu,\n"
               " \"off_bodies_start\": %zu,\n \"off_bodies_end\": %zu,\n \"off_depth\": %zu\n}\n",
               sizeof(Node), alignof(Node), data + offsetof(Data, pos), data + offsetof(Data, mass),
               data + offsetof(Data, quad) + offsetof(Quad, center), data + offsetof(Data, quad) + offsetof(Quad, size),
               offsetof(Node, children), offsetof(Node, next), offsetof(Node, bodies) + offsetof(Range, start),
               offsetof(Node, bodies) + offsetof(Range, end), offsetof(Node, depth));
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s --layout | IN.bin OUT.bin\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 1; }
    std::vector<Body> bodies;
    float rec[3];
    while (fread(rec, sizeof rec, 1, in) == 1) {
        Body b;
        b.pos = Vec2(rec[0], rec[1]);
        b.vel = Vec2::zero();
        b.acc = Vec2::zero();
        b.mass = rec[2];
        b.radius = 0.0f;
        bodies.push_back(b);
    }
    fclose(in);
    Quadtree tree(1.0f, 1.0f, bodies.size());
    tree.build(bodies);
    FILE *out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 1; }
    for (const Node &n : tree.nodes) {
        const float f[6] = {n.data.pos.x, n.data.pos.y, n.data.mass, n.data.quad.center.x, n.data.quad.center.y, n.data.quad.size};
        const uint64_t u[3] = {n.children, n.next, n.depth};
        fwrite(f, sizeof f, 1, out);
        fwrite(u, sizeof u, 1, out);
    }
    fclose(out);
    fprintf(stderr, "%zu bodies, %zu nodes\n", bodies.size(), tree.nodes.size());
    return 0;
}
