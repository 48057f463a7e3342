// Simulation.hpp — C++ adaptor with the reference's `Simulation` surface over the C ABI.
//
// Reference surface being replaced (Nbodysim/headers/Simulation.hpp:49-75):
//   class Simulation { public: float dt; size_t frame; std::vector<Body> bodies; Quadtree quadtree;
//                      Simulation(); void step(); }
//   extern std::atomic<float> SIMULATION_DT;                     Simulation.hpp:16
//
// HOW IT DROPS IN.  Put this directory BEFORE the reference's `headers/` on the include path:
//     g++ -std=c++20 -I nbodysim_amd/host -I include -I Nbodysim/headers  Nbodysim/source/main.cpp ...
// `#include "Simulation.hpp"` (main.cpp:22) then finds this file, and this file uses the reference's OWN
// `Vec2.hpp`, `Body.hpp` and `Node.hpp` (found further down the same include path), so `Vec2` keeps its
// operators and `mag_sq` (main.cpp:108-154), `#include "Vec2.hpp"` (main.cpp:23) is a harmless repeat,
// `std::vector<Node> SHARED_QUADTREE` (main.cpp:41) has its `Node`, and `simulation->quadtree.nodes`
// (main.cpp:626) is this adaptor's node list: empty by default (the force is a direct sum: there is no tree to
// draw), the tree of the step with -DNBODY_TREE=1 -DNBODY_TREE_NODES=1 (below).  The UNMODIFIED main.cpp compiles against this header: INTEGRATION.md §2 gives the
// `g++ -std=c++20 -fsyntax-only` command that checks it.  Without the reference's headers on the path (stand-alone use, e.g.
// sim_thread_example.cpp) minimal layout-identical `Vec2` / `Body` / `Node` are declared here instead.
//
// `Simulation()` starts, like the reference's, from uniform_disc(25000) with epsilon = 1 and the velocity
// clamp + soft boundary of iterate() switched on; a second constructor takes any initial bodies.
// Differences, all deliberate: the force is the direct O(N^2) sum, not Barnes-Hut, and by default
// collide() (Simulation.hpp:72,216-346) is NOT run — bodies with radius > 0 pass through each other, so a run
// from `Simulation()` follows the reference's gravity + clamp + boundary, not its collisions.  Built with
// -DNBODY_COLLIDE=1, reference_params() adds NB_EXTRA_COLLIDE and step() ends with the library's restatement of
// collide() (the pair order and the once-per-pair rule differ from the reference's spatial hash).
// Built with -DNBODY_TREE=1, the force is the reference's own Barnes-Hut walk (NB_FORCE_TREE, theta = 1, Quake rsqrt): the
// reference's accelerations bit for bit.  `quadtree.nodes` is then still not filled (the GUI's tree overlay stays empty, and a frame
// costs no extra call and no extra copy) unless the build also has -DNBODY_TREE_NODES=1: step() and sync() then fill it through
// nb_tree_nodes with the tree of the last force evaluation as the reference's own `Node` records, children of a branch
// consecutive (`nodes[children + i]`), so drawQuadtreeNode (main.cpp:394-475) draws it.  After step() that is the tree of the
// positions before the drift, like the reference's `quadtree.nodes` after its step().  Node indices are the export's canonical
// ones (include/nbody.h), not those of the reference's insertion order.
#pragma once
#include <atomic>
#include <cmath>
#include <cstddef>
#include <future>
#include <mutex>
#include <numbers>
#include <numeric>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "nbody.h"

#if defined(__has_include)
#if __has_include("Vec2.hpp") && __has_include("Body.hpp") && __has_include("Node.hpp")
#define NB_ADAPTOR_REFERENCE_TYPES 1
#endif
#endif

#ifdef NB_ADAPTOR_REFERENCE_TYPES
// the reference's own types (Vec2.hpp:17-357, Body.hpp:6-107, Node.hpp:10-53), by include path — never copied
#include "Body.hpp"
#include "Node.hpp"
#include "Vec2.hpp"
#else
struct alignas(16) Vec2 {                                   // Vec2.hpp:17-20
    float x, y;
    Vec2() noexcept = default;
    constexpr Vec2(float x_, float y_) noexcept : x(x_), y(y_) {}
    static constexpr Vec2 zero() noexcept { return Vec2(0.0f, 0.0f); }
};

struct alignas(16) Body {                                   // Body.hpp:6-17
    Vec2 pos, vel, acc;
    float mass, radius;
    Body() = default;
    Body(Vec2 p, Vec2 v, float m, float r) : pos(p), vel(v), acc(Vec2::zero()), mass(m), radius(r) {}
};

struct Quad {                                               // Quad.hpp: centre and edge length of a cell
    Vec2 center;
    float size;
};

struct Range {                                              // Node.hpp:10-29
    size_t start = 0, end = 0;
};

struct alignas(32) Node {                                   // Node.hpp:31-53
    struct alignas(16) {
        Vec2 pos;
        float mass;
        Quad quad;
    } data{Vec2::zero(), 0.0f, Quad{Vec2::zero(), 0.0f}};
    size_t children = 0, next = 0;
    Range bodies;
    size_t depth = 0;
    bool is_leaf() const { return children == 0; }
    bool is_branch() const { return children != 0; }
    bool is_empty() const { return data.mass == 0.0f; }
};
#endif

#if defined(NBODY_TREE_NODES) && NBODY_TREE_NODES && !(defined(NBODY_TREE) && NBODY_TREE)
#error "NBODY_TREE_NODES=1 needs NBODY_TREE=1: only a Barnes-Hut handle has a tree to export"
#endif

extern std::atomic<float> SIMULATION_DT;  // defined by the application, as in main.cpp:39

static_assert(sizeof(Vec2) == sizeof(nb_vec2) && alignof(Vec2) == 16, "Vec2 layout must match the C ABI (Vec2.hpp:17)");
static_assert(sizeof(Body) == sizeof(nb_body) && offsetof(Body, vel) == offsetof(nb_body, vel) &&
              offsetof(Body, acc) == offsetof(nb_body, acc) && offsetof(Body, mass) == offsetof(nb_body, mass) &&
              offsetof(Body, radius) == offsetof(nb_body, radius), "Body layout must match the C ABI (Body.hpp:6)");

static_assert(sizeof(size_t) == sizeof(uint64_t) && sizeof(Node) == sizeof(nb_tree_node) && alignof(Node) == 32 &&
              offsetof(Node, data.pos) == offsetof(nb_tree_node, pos) && offsetof(Node, data.mass) == offsetof(nb_tree_node, mass) &&
              offsetof(Node, data.quad.center) == offsetof(nb_tree_node, center) &&
              offsetof(Node, data.quad.size) == offsetof(nb_tree_node, size) &&
              offsetof(Node, children) == offsetof(nb_tree_node, children) && offsetof(Node, next) == offsetof(nb_tree_node, next) &&
              offsetof(Node, bodies.start) == offsetof(nb_tree_node, bodies_start) &&
              offsetof(Node, bodies.end) == offsetof(nb_tree_node, bodies_end) && offsetof(Node, depth) == offsetof(nb_tree_node, depth),
              "Node layout must match the C ABI (Node.hpp:31)");

// Stand-in for the reference's `Quadtree quadtree` member (Simulation.hpp:55): the public fields its caller and a
// harness touch.  `nodes` stays empty — main.cpp:626 copies it, main.cpp:737 draws nothing for an empty list — unless the
// build has -DNBODY_TREE=1 -DNBODY_TREE_NODES=1 (fill_nodes, below).
struct DirectSumQuadtree {
    float t_sq = 1.0f;      // Quadtree.hpp:11: theta^2 — unused by a direct sum
    float e_sq = 1.0f;      // Quadtree.hpp:12: epsilon^2 — the softening this handle was created with
    std::vector<Node> nodes;
};

class Simulation {
public:
    float dt = 0.0f;            // unused by the reference too (Simulation.hpp:52)
    size_t frame = 0;
    std::vector<Body> bodies;
    DirectSumQuadtree quadtree;

    // Simulation.hpp:58-65 — the reference's own start (its n, epsilon, ICs; iterate()'s extras on).
    Simulation() : Simulation(uniform_disc(25000), 1.0f, reference_params()) {}

    // Simulation.hpp:347-603, bit-identical bodies (nb_default_ics).
    static std::vector<Body> uniform_disc(size_t n)
    {
        std::vector<Body> b(n);
        check(nb_default_ics(reinterpret_cast<nb_body *>(b.data()), n), "nb_default_ics");
        return b;
    }

    explicit Simulation(std::vector<Body> initial, float epsilon = 1.0f, const nb_params *overrides = nullptr)
        : bodies(std::move(initial))
    {
        nb_params p;
        if (overrides) p = *overrides; else nb_params_default(&p);
        p.eps = epsilon;
        p.dt = SIMULATION_DT.load();
        quadtree.e_sq = epsilon * epsilon;
        sim_ = nb_create(reinterpret_cast<const nb_body *>(bodies.data()), bodies.size(), &p);
        if (!sim_) throw std::runtime_error(std::string("nb_create: ") + nb_last_error());
    }
    ~Simulation()
    {
        if (snapshot_in_flight_) (void)nb_snapshot_wait(sim_);
        nb_destroy(sim_);
    }
    Simulation(const Simulation &) = delete;
    Simulation &operator=(const Simulation &) = delete;

    // HOST MEMORY.  `bodies` is an ordinary std::vector, as in the reference (the caller copies it by value,
    // main.cpp:625); its storage is the heap's, may move whenever the caller assigns or swaps the vector, and shares
    // its first and last page with other heap data.  The adaptor therefore never page-locks it (no hipHostRegister of
    // memory it does not own page-wise, nothing to unregister after a reallocation): nb_sync / nb_snapshot_wait fill it
    // from the library's own page-locked staging buffer, the host copy pipelined against the DMA.

    // Simulation.hpp:67-75 — on return `bodies` is coherent (pos, vel, acc, mass, radius).
    // `bodies` is public in the reference and stays public here, but the device state has a fixed size: a caller
    // that resized the vector gets an exception, not an out-of-bounds write (host edits go through upload()).
    void step()
    {
        check_size();
        if (snapshot_in_flight_) { check(nb_snapshot_wait(sim_), "nb_snapshot_wait"); snapshot_in_flight_ = false; }
        const float current_dt = SIMULATION_DT.load();
        check(nb_step(sim_, current_dt, 1), "nb_step");
        check(nb_sync(sim_, reinterpret_cast<nb_body *>(bodies.data())), "nb_sync");
        fill_nodes();
        ++frame;
    }

    // Pipelined form of step() for a viewer that can draw one frame late: advances one step and returns with `bodies`
    // holding the state after the PREVIOUS call's step.  The device-to-host copy of frame k (16.8 MB at N = 262 144)
    // runs on a copy stream into the library's page-locked staging buffer while the force of step k + 1 computes
    // (nb_snapshot_begin); nb_snapshot_wait then moves it into a PRIVATE vector — also while step k + 1 is running,
    // because that step was enqueued first — which is swapped with `bodies` (O(1)).  The destination of a snapshot in
    // flight is never the public vector, whose storage the caller may move at any time.  Call sync() to catch up.
// It does NOT fill `quadtree.nodes`, with or without NBODY_TREE_NODES: `bodies` is one frame late here while the tree of the
// handle is not, and a tree drawn over the bodies of another frame is worse than none.
    void step_overlapped()
    {
        check_size();
        if (back_.size() != bodies.size()) {
            if (snapshot_in_flight_) { check(nb_snapshot_wait(sim_), "nb_snapshot_wait"); snapshot_in_flight_ = false; }
            back_.assign(bodies.size(), Body());
        }
        check(nb_step(sim_, SIMULATION_DT.load(), 1), "nb_step");                                   // enqueue step k + 1
        if (snapshot_in_flight_) {
            check(nb_snapshot_wait(sim_), "nb_snapshot_wait");                                      // frame k -> back_ (GPU busy with k + 1)
            bodies.swap(back_);
        }
        check(nb_snapshot_begin(sim_, reinterpret_cast<nb_body *>(back_.data())), "nb_snapshot_begin");   // frame k + 1 follows it
        snapshot_in_flight_ = true;
        ++frame;
    }

    // Throughput form: k steps without refreshing `bodies` (call sync() when a snapshot is wanted).
    void advance(int k)
    {
        check(nb_step(sim_, SIMULATION_DT.load(), k), "nb_step");
        frame += (size_t)k;
    }
    void sync()
    {
        check_size();
        if (snapshot_in_flight_) { check(nb_snapshot_wait(sim_), "nb_snapshot_wait"); snapshot_in_flight_ = false; }
        check(nb_sync(sim_, reinterpret_cast<nb_body *>(bodies.data())), "nb_sync");
        fill_nodes();
    }
    // After editing `bodies` in place on the host (same count).
    void upload() { check_size(); check(nb_upload(sim_, reinterpret_cast<const nb_body *>(bodies.data())), "nb_upload"); }
    // The frame as an image instead of as bodies (nb_raster, include/nbody.h): bodies, and mass in quanta, per pixel of `view`, binned
    // on the device at the positions of the work enqueued so far; `bodies` is not refreshed and need not be.  Replaces the per-body draw
    // loop of main.cpp:745-835 by one texture upload.  Either plane may be null, not both; each holds view.width * view.height elements.
    void raster(const nb_view &view, uint32_t *count, float *mass) { check(nb_raster(sim_, &view, count, mass), "nb_raster"); }
    // The potential of every body (nb_potentials, include/nbody.h) at the positions of the work enqueued so far: phi holds bodies.size()
    // doubles; with the velocities of `bodies` after step(): binding energy of body i = |vel_i|^2 / 2 + phi[i].
    void potentials(double *phi) { check(nb_potentials(sim_, phi), "nb_potentials"); }
    // Who is near every body (nb_neighbors, include/nbody.h), at the positions of the work enqueued so far: for drawConnections
    // (main.cpp:233-386) call it with MAX_DISTANCE and MAX_CONNECTIONS; row i of idx then holds the k nearest bodies within `radius` of
    // bodies[i], nearest first, padded with NB_NO_NEIGHBOR; dist2 their squared distances, count[i] all of them.  idx and dist2 hold
    // bodies.size() * k entries, count bodies.size(); any may be null, not all three.
    void neighbors(float radius, uint32_t k, uint32_t *idx, float *dist2, uint32_t *count)
    {
        check(nb_neighbors(sim_, radius, k, idx, dist2, count), "nb_neighbors");
    }
    // Which bodies form a clump (nb_groups, include/nbody.h), at the positions of the work enqueued so far: the friends-of-friends
    // groups at linking length `radius`.  label[i] is the smallest index of the group of bodies[i], size[i] its member count, *ngroups
    // the number of groups; label and size hold bodies.size() entries; any may be null, not all three.
    void groups(float radius, uint32_t *label, uint32_t *size, uint64_t *ngroups)
    {
        check(nb_groups(sim_, radius, label, size, ngroups), "nb_groups");
    }
    // Unbinding (nb_group_binding, include/nbody.h), at the positions of the work enqueued so far: for every group of groups(radius)
    // with at least min_members bodies, phi[i] = the potential of bodies[i] due to the other members of its own group and e[i] = its
    // energy in the group's rest frame (bound when e[i] < 0; NaN for a body of a smaller group), and one nb_group_energy per group:
    // bound members, the most bound one (the centre), the self-potential energy.  phi and e hold bodies.size() doubles, out `capacity`
    // records; any may be null; all three null asks for the number of groups only.  Returns that number.
    size_t group_binding(float radius, uint32_t min_members, double *phi, double *e, nb_group_energy *out, size_t capacity)
    {
        size_t count = 0;
        check(nb_group_binding(sim_, radius, min_members, phi, e, out, capacity, &count), "nb_group_binding");
        return count;
    }
    // The histogram of pair separations (nb_pair_counts, include/nbody.h), at the positions of the work enqueued so far: counts[b] is
    // the number of unordered pairs of bodies with edges[b] <= distance < edges[b + 1] (squares compared in float); edges holds
    // nbins + 1 ascending values, counts nbins entries, nbins <= NB_PAIR_BINS_MAX.
    void pair_counts(const float *edges, uint32_t nbins, uint64_t *counts)
    {
        check(nb_pair_counts(sim_, edges, nbins, counts), "nb_pair_counts");
    }
    // Shell sums about `ncenters` points (nb_radial_profiles, include/nbody.h), at the positions of the work enqueued so far:
    // out[c * nbins + b] is the count and the fp64 mass and velocity moments of the bodies with edges[b] <= |x - centre c| < edges[b + 1]
    // (squares compared in float).  centers holds `dims` floats a centre, vcenters (may be null: zero) as many doubles.
    void radial_profiles(const float *centers, const double *vcenters, size_t ncenters, const float *edges, uint32_t nbins, nb_shell *out)
    {
        check(nb_radial_profiles(sim_, centers, vcenters, ncenters, edges, nbins, out), "nb_radial_profiles");
    }
    nb_sim *handle() { return sim_; }

private:
    static const nb_params *reference_params()
    {
        static nb_params p;
        nb_params_default(&p);
        p.extras = NB_EXTRA_VCLAMP | NB_EXTRA_BOUNDARY;     // Simulation.hpp:133-155
#if defined(NBODY_COLLIDE) && NBODY_COLLIDE
        p.extras |= NB_EXTRA_COLLIDE;                       // Simulation.hpp:72,216-346
#endif
#if defined(NBODY_TREE) && NBODY_TREE
        p.force = NB_FORCE_TREE;                            // Simulation.hpp:176-214: Barnes-Hut, theta = 1 (:59), the reference's
        p.rsqrt_mode = NB_RSQRT_QUAKE;                      // own arithmetic (Quadtree.hpp:106-111): its frames bit for bit
#endif
        return &p;
    }
    // -DNBODY_TREE=1 -DNBODY_TREE_NODES=1: `quadtree.nodes` = the tree of the last build (nb_tree_nodes: the count, resize, then the
    // records written in place).  Like `bodies` the vector is the heap's and is never page-locked: the library stages the copy.
    // Any other build: nothing, not even a call.
    void fill_nodes()
    {
#if defined(NBODY_TREE_NODES) && NBODY_TREE_NODES
        size_t count = 0;
        check(nb_tree_nodes(sim_, nullptr, 0, &count), "nb_tree_nodes");
        quadtree.nodes.resize(count);
        if (count) check(nb_tree_nodes(sim_, reinterpret_cast<nb_tree_node *>(quadtree.nodes.data()), count, &count), "nb_tree_nodes");
#endif
    }
    static void check(int rc, const char *what)
    {
        if (rc != NB_OK) throw std::runtime_error(std::string(what) + ": " + nb_last_error());
    }
    void check_size() const
    {
        if (bodies.size() != nb_count(sim_))
            throw std::length_error("Simulation::bodies was resized (" + std::to_string(bodies.size()) + " != " +
                                    std::to_string(nb_count(sim_)) + "): the device state has a fixed body count");
    }
    nb_sim *sim_ = nullptr;
    std::vector<Body> back_;            // step_overlapped(): private destination of the snapshot in flight
    bool snapshot_in_flight_ = false;
};
