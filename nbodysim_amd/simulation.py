"""Host-side mirror of the reference's ``Simulation`` surface over the C ABI.

Reference (``Nbodysim/headers/Simulation.hpp:49-75``)::

    class Simulation { public: float dt; size_t frame; std::vector<Body> bodies;
                       Quadtree quadtree; Simulation(); void step(); };
    extern std::atomic<float> SIMULATION_DT;          // main.cpp:39, read once per step (:69)

Here ``Simulation(bodies, ...)`` takes the initial bodies instead of the
hard-coded ``uniform_disc(25000)``; ``step()`` advances one step with the
module-level ``SIMULATION_DT`` (or an explicit dt) and leaves ``bodies``
coherent, like the reference's ``step()`` does for its only caller
(``simulation_thread``, main.cpp:612-635).  ``advance(nsteps)`` is the
throughput form: it only enqueues work and does not refresh ``bodies``.

All compute happens in ``libnbody_hip.so`` on the GPU; nothing here computes
forces.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L

#: the reference's global time step (``std::atomic<float> SIMULATION_DT{0.01f}``, main.cpp:39)
SIMULATION_DT: float = 0.01


class Simulation:
    """One ``nb_sim`` handle plus the host ``bodies`` view."""

    def __init__(
        self,
        bodies: np.ndarray,
        eps: float = 1.0,           # Simulation.hpp:59 -> Quadtree(theta=1, epsilon=1)
        precision: str = "fp32",
        rsqrt: str = "exact",
        order: str = "tiled",
        integrator: str = "kick_drift",
        extras: int = 0,
        device: int = -1,
        j_slices: int = 0,
        i_begin: int = 0,
        i_count: int = 0,
        stream: Optional[int] = None,
        pos_buffers: Optional[tuple] = None,
        shard_rank: int = 0,
        shard_world: int = 0,
        acc_buffers: Optional[tuple] = None,
        dims: int = 2,
        symmetry: bool = True,
        uniform_mass: bool = True,
        guided_tail: bool = True,
        sym_chunks_per_item: int = 0,
        sym_aux_stream: int = 0,
        sym_late_us: float = 0.0,
        lanes_p: int = 0,
        sym_tail: Optional[tuple] = None,
        shard_allreduce: bool = False,
        first_frame: int = 0,
        shard_single: bool = False,
        mass_scaling=False,
        sym_chunk_pairs: int = 0,
        sym_tile: int = 0,
        pos_rows: int = 0,
        static_items: bool = False,
        collide: bool = False,
        force: str = "direct",
        theta: float = 1.0,
        library=None,
        tree_leaves: bool = False,
        tree_quadrupole: bool = False,
        tree_energy: bool = False,
        tree_alpha: Optional[float] = None,
        body_order: Optional[bool] = None,
    ):
        """``integrator``: "kick_drift" (the reference's, first order), "kdk", or one of the composed integrators that every unsharded
        handle takes, tree handles included: "dkd" (drift-kick-drift leapfrog: second order, reversible, one force evaluation per step)
        and "fr4" (Forest-Ruth, fourth order, three evaluations per step; no ``extras``) — NB_INTEGRATOR_DKD / _FR4 of include/nbody.h.
        "hermite4": the 4th-order Hermite predictor-corrector, one evaluation of acceleration and jerk per step (NB_INTEGRATOR_HERMITE4:
        unsharded direct-sum handles, tiled sum, hardware rsqrt, no ``extras``; ``dt`` may change from step to step; see ``jerks``).
        The last arguments (from ``uniform_mass`` on) are ``nb_params.flags`` and the launch-geometry tuning fields
        (0 / True = the library's automatic choice); the library reads no environment variables.  ``mass_scaling``: False / None
        (default) = both per-pair mass multiplies, True = fold the masses into the pair geometry wherever representable
        (include/nbody.h, NB_FLAG_MASS_SCALING), "measured" = the library measures at upload whether folding is harmless for
        these bodies and folds only then (NB_FLAG_MASS_SCALING_MEASURED).  ``collide``: end every step with the reference's
        hard-sphere collisions (adds NB_EXTRA_COLLIDE to ``extras``; unsharded 2-D kick-drift only).  ``force``: "direct" (every pair) or "tree" (the reference's
        Barnes-Hut quadtree with opening parameter ``theta``, NB_FORCE_TREE; unsharded 2-D fp32 with the kick-drift, DKD or FR4 integrator only).  ``tree_leaves``
        (``force="tree"`` only, ValueError otherwise): the convergent tree force, NB_FLAG_TREE_LEAVES — leaves that are not accepted
        contribute, so the result tends to the direct sum as ``theta`` -> 0; not the reference's arithmetic.  ``tree_quadrupole``
        (``force="tree"`` with ``tree_leaves=True`` only, ValueError otherwise): accepted cells add their second moment,
        NB_FLAG_TREE_QUADRUPOLE — the same walk, a smaller error at the same ``theta``, +256 bytes per body.  ``tree_energy``
        (``force="tree"`` with ``tree_leaves=True`` only, ValueError otherwise): ``energy()`` walks the tree instead of sweeping all
        pairs, NB_FLAG_TREE_ENERGY — O(n log n), the same pairs, the error of the force walk at this ``theta`` (``theta=0`` is the
        direct energy); it rebuilds the tree and leaves the trajectory alone.  ``tree_alpha`` (None or a float; ``force="tree"`` with
        ``tree_leaves=True`` only, ValueError otherwise): NB_FLAG_TREE_RELATIVE — a cell is accepted only if it also passes
        m size^2 / d^4 < ``tree_alpha`` |a_prev| with the body's own last acceleration (``theta`` stays the cap; fresh initial
        conditions have a_prev = 0, so call ``accelerations()`` once before stepping to have the test active from step 1);
        ``set_tree_alpha`` changes it between steps, 0 switches it off.  ``body_order``: None = the library's rule (the whole-system
        symmetric kernel sweeps the bodies along a Morton curve at 131 072 .. 262 144 bodies), True = NB_FLAG_BODY_ORDER (at any size), False =
        NB_FLAG_NO_BODY_ORDER (the caller's order); results differ by summation order only, ``describe()`` says which.  ``library``: another
        build of the library bound with ``_lib.bind`` (the tests' -DNB_TEST_HOOKS build); default the product."""
        if tree_leaves and force != "tree":
            raise ValueError('tree_leaves=True needs force="tree" (NB_FLAG_TREE_LEAVES selects a walk of the Barnes-Hut force)')
        if tree_quadrupole and not (force == "tree" and tree_leaves):
            raise ValueError('tree_quadrupole=True needs force="tree" and tree_leaves=True (NB_FLAG_TREE_QUADRUPOLE adds a term to the '
                             "accepted cells of the convergent Barnes-Hut force)")
        if tree_energy and not (force == "tree" and tree_leaves):
            raise ValueError('tree_energy=True needs force="tree" and tree_leaves=True (NB_FLAG_TREE_ENERGY makes energy() walk the tree '
                             "of the convergent Barnes-Hut force)")
        if tree_alpha is not None and not (force == "tree" and tree_leaves):
            raise ValueError('tree_alpha needs force="tree" and tree_leaves=True (NB_FLAG_TREE_RELATIVE adds an acceleration-relative '
                             "opening test to the walks of the convergent Barnes-Hut force)")
        lib = library if library is not None else L.load()
        if bodies.dtype not in (L.BODY_DTYPE, L.BODY3_DTYPE):
            raise TypeError("bodies must be a numpy array of nbodysim_amd.BODY_DTYPE (64-byte Body records)")
        bodies = np.ascontiguousarray(bodies)
        view = L.BODY3_DTYPE if dims == 3 else L.BODY_DTYPE
        bodies = bodies.view(view)
        p = L.nb_params()
        lib.nb_params_default(C.byref(p))
        p.eps = eps
        p.dt = SIMULATION_DT
        p.precision = {"fp32": L.NB_FP32, "fp64": L.NB_FP64}[precision]
        p.rsqrt_mode = {"exact": L.NB_RSQRT_EXACT, "quake": L.NB_RSQRT_QUAKE}[rsqrt]
        p.sum_order = {"tiled": L.NB_SUM_TILED, "sequential": L.NB_SUM_SEQUENTIAL}[order]
        p.integrator = {"kick_drift": L.NB_INTEGRATOR_KICK_DRIFT, "kdk": L.NB_INTEGRATOR_KDK, "dkd": L.NB_INTEGRATOR_DKD,
                        "fr4": L.NB_INTEGRATOR_FR4, "hermite4": L.NB_INTEGRATOR_HERMITE4}[integrator]
        p.extras = extras | (L.NB_EXTRA_COLLIDE if collide else 0)
        p.device = device
        p.j_slices = j_slices
        p.i_begin = i_begin
        p.i_count = i_count
        if stream is not None:
            p.stream = stream
        if pos_buffers is not None:
            p.pos_buffers[0], p.pos_buffers[1] = pos_buffers
        p.dims = dims
        p.flags = ((0 if symmetry else L.NB_FLAG_NO_SYMMETRY) | (0 if uniform_mass else L.NB_FLAG_NO_UNIFORM_MASS)
                   | (0 if guided_tail else L.NB_FLAG_NO_GUIDED_TAIL) | (L.NB_FLAG_SHARD_ALLREDUCE if shard_allreduce else 0)
                   | (L.NB_FLAG_SHARD_SINGLE if shard_single else 0)
                   | (L.NB_FLAG_MASS_SCALING_MEASURED if mass_scaling == "measured" else L.NB_FLAG_MASS_SCALING if mass_scaling is True
                      else L.NB_FLAG_NO_MASS_SCALING if mass_scaling is False else 0)
                   | (L.NB_FLAG_STATIC_ITEMS if static_items else 0) | (L.NB_FLAG_TREE_LEAVES if tree_leaves else 0)
                   | (L.NB_FLAG_TREE_QUADRUPOLE if tree_quadrupole else 0) | (L.NB_FLAG_TREE_ENERGY if tree_energy else 0)
                   | (L.NB_FLAG_TREE_RELATIVE if tree_alpha is not None else 0)
                   | (L.NB_FLAG_BODY_ORDER if body_order is True else L.NB_FLAG_NO_BODY_ORDER if body_order is False else 0))
        p.sym_chunks_per_item, p.sym_aux_stream, p.sym_late_us, p.lanes_p = sym_chunks_per_item, sym_aux_stream, sym_late_us, lanes_p
        if sym_tail is not None:
            p.sym_tail[0], p.sym_tail[1], p.sym_tail[2] = sym_tail
        p.first_frame = first_frame
        p.sym_chunk_pairs = sym_chunk_pairs
        p.sym_tile = sym_tile
        p.pos_rows = pos_rows
        p.force = {"direct": L.NB_FORCE_DIRECT, "tree": L.NB_FORCE_TREE}[force]
        p.theta = theta
        p.shard_rank, p.shard_world = shard_rank, shard_world
        if acc_buffers is not None:
            p.acc_buffers[0], p.acc_buffers[1] = acc_buffers
        self._lib = lib
        self._params = p
        self._h = lib.nb_create(bodies.ctypes.data, bodies.shape[0], C.byref(p))
        if not self._h:
            raise L.NBodyError("nb_create", L.last_error_code(lib), L.last_error(lib))
        if tree_alpha is not None:
            rc = lib.nb_tree_alpha(self._h, tree_alpha)
            if rc:
                err = L.NBodyError("nb_tree_alpha", L.last_error_code(lib), L.last_error(lib))
                lib.nb_destroy(self._h)
                self._h = None
                raise err
        self.n = int(lib.nb_count(self._h))
        self.i_begin = int(lib.nb_owned_begin(self._h))
        self.i_count = int(lib.nb_owned_count(self._h))
        #: host view of the owned block; refreshed by step() / sync()
        self.bodies = np.frombuffer(bodies[self.i_begin : self.i_begin + self.i_count].tobytes(), dtype=view).copy()

    # -- reference surface ---------------------------------------------------
    @property
    def frame(self) -> int:
        return int(self._lib.nb_frame(self._h))

    def step(self, dt: Optional[float] = None) -> None:
        """``Simulation::step()``: one step, then ``bodies`` is coherent."""
        L.check("nb_step", self._lib.nb_step(self._h, SIMULATION_DT if dt is None else dt, 1), self._lib)
        self.sync()

    # -- throughput / build-defined surface ------------------------------------
    def advance(self, nsteps: int, dt: Optional[float] = None) -> None:
        """Enqueue nsteps steps; does not wait and does not refresh ``bodies``."""
        L.check("nb_step", self._lib.nb_step(self._h, SIMULATION_DT if dt is None else dt, nsteps), self._lib)

    def wait(self) -> None:
        L.check("nb_wait", self._lib.nb_wait(self._h), self._lib)

    def sync(self) -> np.ndarray:
        L.check("nb_sync", self._lib.nb_sync(self._h, self.bodies.ctypes.data), self._lib)
        return self.bodies

    def snapshot_begin(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Pipelined ``sync``: start copying the state as of the work enqueued so far into ``out`` (default:
        ``self.bodies``) and return at once; steps enqueued afterwards overlap the transfer.  Pair with ``snapshot_wait``."""
        out = self.bodies if out is None else out
        L.check("nb_snapshot_begin", self._lib.nb_snapshot_begin(self._h, out.ctypes.data), self._lib)
        return out

    def snapshot_wait(self) -> None:
        L.check("nb_snapshot_wait", self._lib.nb_snapshot_wait(self._h), self._lib)

    def positions(self) -> np.ndarray:
        out = np.empty((self.i_count, 3 if self._params.dims == 3 else 2), dtype=np.float32)
        L.check("nb_sync_positions", self._lib.nb_sync_positions(self._h, out.ctypes.data), self._lib)
        return out

    def upload(self, bodies: np.ndarray) -> None:
        if bodies.dtype != L.BODY_DTYPE or bodies.shape[0] != self.n:
            raise ValueError("upload needs the n bodies of the whole system")
        bodies = np.ascontiguousarray(bodies)
        L.check("nb_upload", self._lib.nb_upload(self._h, bodies.ctypes.data), self._lib)

    def accelerations(self) -> np.ndarray:
        """Evaluate a(x) at the current positions (``attract()`` as a direct sum)."""
        L.check("nb_accelerations", self._lib.nb_accelerations(self._h), self._lib)
        return self.sync()["acc"].copy()

    def energy(self) -> tuple:
        k, u = C.c_double(), C.c_double()
        L.check("nb_energy", self._lib.nb_energy(self._h, C.byref(k), C.byref(u)), self._lib)
        return k.value, u.value

    def momentum(self) -> tuple:
        """((px, py, pz), Lz): total linear momentum (``Body::momentum``, Body.hpp:103-106, summed; fp64 on the
        device) and angular momentum about the origin of the owned block."""
        p, lz = (C.c_double * 3)(), C.c_double()
        L.check("nb_momentum", self._lib.nb_momentum(self._h, p, C.byref(lz)), self._lib)
        return (p[0], p[1], p[2]), lz.value

    def potentials(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The potential of every owned body, ``phi_i = -sum_{j != i} m_j / sqrt(r_ij^2 + eps^2)`` (``nb_potentials``; synchronises):
        float64 of shape ``(i_count,)``; the binding energy of body i is ``v_i^2 / 2 + phi_i``.  ``out``: a writeable C-contiguous
        float64 array of that shape (one over ``nb_host_alloc`` memory is written by the copy engine directly); default a new array."""
        if out is None:
            out = np.empty(self.i_count, dtype=np.float64)
        elif (not isinstance(out, np.ndarray) or out.dtype != np.float64 or out.shape != (self.i_count,) or not out.flags.c_contiguous
              or not out.flags.writeable):
            raise TypeError(f"out must be a writeable C-contiguous ({self.i_count},) numpy array of float64")
        L.check("nb_potentials", self._lib.nb_potentials(self._h, out.ctypes.data), self._lib)
        return out

    def collision_stats(self) -> dict:
        """Counters of the collision path (``nb_collision_stats``; synchronises): pairs of the last step, pairs resolved since
        creation, resolution rounds of the last step, steps that were over the pair capacity.  All 0 without ``collide``."""
        last, total, ovf = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rounds = C.c_uint32()
        L.check("nb_collision_stats", self._lib.nb_collision_stats(self._h, C.byref(last), C.byref(total), C.byref(rounds), C.byref(ovf)),
                self._lib)
        return {"pairs_last_step": int(last.value), "pairs_total": int(total.value), "rounds_last_step": int(rounds.value),
                "overflow_steps": int(ovf.value)}

    def collide_capacity(self, max_pairs: int) -> None:
        """Set the pair capacity of the collision path (``nb_collide_capacity``)."""
        L.check("nb_collide_capacity", self._lib.nb_collide_capacity(self._h, max_pairs), self._lib)

    def tree_stats(self) -> dict:
        """Figures of the last Barnes-Hut force evaluation (``nb_tree_stats``; synchronises): nodes, deepest leaf, evaluations
        that failed (node capacity, depth cap) since creation."""
        nodes, ovf = C.c_uint64(), C.c_uint64()
        depth = C.c_uint32()
        L.check("nb_tree_stats", self._lib.nb_tree_stats(self._h, C.byref(nodes), C.byref(depth), C.byref(ovf)), self._lib)
        return {"nodes": int(nodes.value), "max_depth": int(depth.value), "overflow_steps": int(ovf.value)}

    def tree_nodes(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The tree of the most recent build as the reference's ``quadtree.nodes`` (``nb_tree_nodes``; synchronises): an array of
        ``NODE_DTYPE`` records in reference form (include/nbody.h).  The count is queried first; ``out`` (a contiguous
        ``NODE_DTYPE`` array, e.g. a view of ``nb_host_alloc`` memory) must hold at least that many records and the view of its
        filled part is returned; default a new array.  Empty before any build."""
        cnt = C.c_size_t()
        L.check("nb_tree_nodes", self._lib.nb_tree_nodes(self._h, None, 0, C.byref(cnt)), self._lib)
        if out is None:
            out = L.nodes_array(cnt.value)
        elif out.dtype != L.NODE_DTYPE or out.ndim != 1 or not out.flags.c_contiguous:
            raise TypeError("out must be a contiguous 1-D numpy array of nbodysim_amd.NODE_DTYPE (128-byte Node records)")
        if cnt.value:
            L.check("nb_tree_nodes", self._lib.nb_tree_nodes(self._h, out.ctypes.data, out.shape[0], C.byref(cnt)), self._lib)
        return out[: cnt.value]

    def raster(self, width: int, height: int, center=(0.0, 0.0), scale: float = 1.0, mass_quantum: Optional[float] = None, out=None):
        """The owned bodies binned into a ``(height, width)`` image on the device (``nb_raster``; synchronises): the reference's
        worldToScreen with ``center`` and ``scale``, pixel ``[int(sy), int(sx)]``.  Returns the uint32 count plane; with a
        ``mass_quantum`` returns ``(count, mass)``, mass a float32 plane summed in whole quanta (include/nbody.h).  ``out``: a
        C-contiguous ``(height, width)`` uint32 array for the counts, or a pair ``(count, mass)`` of which either may be None: a
        plane given as None in the pair is not computed and None is returned in its place (``mass`` needs a ``mass_quantum``).
        Arrays over ``nb_host_alloc`` memory are written by the copy engine directly."""
        # refused here, by name, before anything is allocated (the c_uint32 fields of nb_view would wrap a negative silently)
        for name, val in (("width", width), ("height", height)):
            if not 1 <= val <= 16384:
                raise ValueError(f"raster: {name} must be 1 .. 16384 (got {val})")
        if width * height > 1 << 24:
            raise ValueError(f"raster: width * height must be <= 2^24 (got {width} x {height})")
        count = mass = None
        want_count, want_mass = True, mass_quantum is not None
        if isinstance(out, (tuple, list)):
            count, mass = out
            want_count = count is not None
            want_mass = mass is not None
            if want_mass and mass_quantum is None:
                raise ValueError("a mass plane needs a mass_quantum")
        elif out is not None:
            count = out
        for name, a, dt in (("count", count, np.uint32), ("mass", mass, np.float32)):
            if a is not None and (not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != (height, width) or not a.flags.c_contiguous
                                  or not a.flags.writeable):
                raise TypeError(f"out: the {name} plane must be a writeable C-contiguous ({height}, {width}) numpy array of {np.dtype(dt).name}")
        if want_count and count is None:
            count = np.empty((height, width), dtype=np.uint32)
        if want_mass and mass is None:
            mass = np.empty((height, width), dtype=np.float32)
        v = L.nb_view()
        v.struct_size = C.sizeof(L.nb_view)
        v.width, v.height = width, height
        v.center_x, v.center_y = center
        v.scale = scale
        v.mass_quantum = 0.0 if mass_quantum is None else mass_quantum
        L.check("nb_raster", self._lib.nb_raster(self._h, C.byref(v), count.ctypes.data if want_count and count is not None else None,
                                                 mass.ctypes.data if want_mass and mass is not None else None), self._lib)
        if isinstance(out, (tuple, list)) or mass_quantum is not None:
            return (count if want_count else None), (mass if want_mass else None)
        return count

    def neighbors(self, radius: float, k: int, dist2: bool = False, count: bool = False):
        """The ``k`` nearest bodies within ``radius`` of every owned body, found on the device (``nb_neighbors``; synchronises): j is a
        neighbour of i when ``j != i`` and the fp32 ``dx*dx + dy*dy < radius*radius``.  Returns the ``(i_count, k)`` uint32 array of
        global body indices in ascending order of (d2, index), padded with ``NB_NO_NEIGHBOR``; with ``dist2`` also the float32 d2 of
        the same shape, padded with +inf; with ``count`` also the uint32 number of ALL neighbours of every owned body, not capped
        at ``k``: ``idx``, ``(idx, d2)``, ``(idx, count)`` or ``(idx, d2, count)``.  ``k = 0`` is the count-only call and returns
        the counts alone."""
        if not 0 <= k <= 32:
            raise ValueError(f"neighbors: k must be 1 .. 32, or 0 for the counts alone (got {k})")
        rows = k > 0
        idx = np.empty((self.i_count, k), dtype=np.uint32) if rows else None
        d2 = np.empty((self.i_count, k), dtype=np.float32) if rows and dist2 else None
        cnt = np.empty(self.i_count, dtype=np.uint32) if count or not rows else None
        L.check("nb_neighbors", self._lib.nb_neighbors(self._h, radius, k, *(a.ctypes.data if a is not None else None for a in (idx, d2, cnt))),
                self._lib)
        if not rows:
            return cnt
        out = tuple(a for a in (idx, d2, cnt) if a is not None)
        return out[0] if len(out) == 1 else out

    def groups(self, radius: float, size: bool = False, ngroups: bool = False):
        """The friends-of-friends groups of the bodies at linking length ``radius``, found on the device (``nb_groups``;
        synchronises): i and j are linked when ``j != i`` and the fp32 ``dx*dx + dy*dy < radius*radius``; the groups are the
        connected components over all n bodies.  Returns the ``(i_count,)`` uint32 labels of the owned block, each the smallest
        global body index of its group; with ``size`` also the uint32 member count of every owned body's group; with ``ngroups``
        also the number of groups among all n bodies as an int: ``label``, ``(label, size)``, ``(label, ngroups)`` or
        ``(label, size, ngroups)``."""
        label = np.empty(self.i_count, dtype=np.uint32)
        sizes = np.empty(self.i_count, dtype=np.uint32) if size else None
        count = C.c_uint64(0)
        L.check("nb_groups", self._lib.nb_groups(self._h, radius, label.ctypes.data, sizes.ctypes.data if size else None,
                                                 C.byref(count) if ngroups else None), self._lib)
        out = (label,) + ((sizes,) if size else ()) + ((int(count.value),) if ngroups else ())
        return out[0] if len(out) == 1 else out

    def group_catalog(self, radius: float, min_members: int = 2, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The catalogue of the friends-of-friends groups at linking length ``radius`` with at least ``min_members`` bodies, reduced on
        the device (``nb_group_catalog``; synchronises): a ``GROUP_DTYPE`` array in ascending order of ``label`` with ``members``,
        ``mass``, the centre of mass ``pos``, the mean velocity ``vel``, the velocity dispersion ``sigma2`` and the radius ``r_max`` of
        every group (include/nbody.h has the definitions).  The count is queried first, then the records are filled.  ``out``: a
        writeable C-contiguous 1-D ``GROUP_DTYPE`` array that holds at least that many records (one over ``nb_host_alloc`` memory is
        written by the copy engine directly); the view of its filled part is returned; default a new array.  The handle must own all
        n bodies."""
        if not 1 <= min_members <= 0xFFFFFFFF:
            raise ValueError(f"group_catalog: min_members must be 1 .. 2^32 - 1 (got {min_members})")
        if out is not None and (not isinstance(out, np.ndarray) or out.dtype != L.GROUP_DTYPE or out.ndim != 1 or not out.flags.c_contiguous
                                or not out.flags.writeable):
            raise TypeError("out must be a writeable C-contiguous 1-D numpy array of nbodysim_amd.GROUP_DTYPE (80-byte nb_group records)")
        cnt = C.c_size_t()
        L.check("nb_group_catalog", self._lib.nb_group_catalog(self._h, radius, min_members, None, 0, C.byref(cnt)), self._lib)
        if out is None:
            out = np.zeros(cnt.value, dtype=L.GROUP_DTYPE)
        if cnt.value:
            L.check("nb_group_catalog", self._lib.nb_group_catalog(self._h, radius, min_members, out.ctypes.data, out.shape[0], C.byref(cnt)),
                    self._lib)
        return out[: cnt.value]

    def group_binding(self, radius: float, min_members: int = 2, phi: bool = False, e: bool = True, records: bool = True):
        """Unbinding on the device (``nb_group_binding``; synchronises), for the groups of ``group_catalog(radius, min_members)``:
        ``phi[i]``, the potential of body i due to the other members of its own group; ``e[i] = |v_i - vel_G|^2 / 2 + phi[i]``, its
        energy in the group's rest frame (bound when ``e[i] < 0``); both ``(n,)`` float64, NaN for a body whose group is not kept; and a
        ``GROUP_ENERGY_DTYPE`` array, row r for the group of row r of the catalogue: ``label``, ``members``, ``bound``, ``most_bound``
        (the global index of the member with the smallest e: the group's centre), ``e_min`` and ``potential`` (the self-potential
        energy).  Returns what was asked for, in the order phi, e, records: one array, or a tuple; with none of the three the number
        of groups.  The count is queried first, then one filling call runs the sweep.  The handle must own all n bodies."""
        if not 1 <= min_members <= 0xFFFFFFFF:
            raise ValueError(f"group_binding: min_members must be 1 .. 2^32 - 1 (got {min_members})")
        cnt = C.c_size_t()
        L.check("nb_group_binding", self._lib.nb_group_binding(self._h, radius, min_members, None, None, None, 0, C.byref(cnt)), self._lib)
        if not (phi or e or records):
            return int(cnt.value)
        planes = [np.empty(self.n, dtype=np.float64) if want else None for want in (phi, e)]
        rec = np.zeros(cnt.value, dtype=L.GROUP_ENERGY_DTYPE) if records else None
        L.check("nb_group_binding", self._lib.nb_group_binding(self._h, radius, min_members, *(a.ctypes.data if a is not None else None for a in planes),
                                                               rec.ctypes.data if records and cnt.value else None, cnt.value, C.byref(cnt)), self._lib)
        out = tuple(a for a in planes if a is not None) + ((rec[: cnt.value],) if records else ())
        return out[0] if len(out) == 1 else out

    def pair_counts(self, edges) -> np.ndarray:
        """The histogram of pair separations DD(r), counted on the device (``nb_pair_counts``; synchronises): ``edges`` are the
        ``nbins + 1`` strictly ascending bin edges, 1 <= nbins <= 64, passed on as float32; bin b holds the unordered pairs {i, j} with
        ``edges[b]**2 <= dx*dx + dy*dy < edges[b+1]**2`` in fp32, each pair once.  Returns the ``(nbins,)`` uint64 counts, exact.  A
        handle that owns a block counts the pairs whose lower global index lies in it, so the counts of the ranks of a sharded run
        add up to the whole.  The edges are validated by the library (include/nbody.h has the rules)."""
        e = np.ascontiguousarray(edges, dtype=np.float32)
        if e.ndim != 1 or e.size < 2:
            raise ValueError("pair_counts: edges must be a 1-D sequence of at least two values")
        counts = np.zeros(e.size - 1, dtype=np.uint64)
        L.check("nb_pair_counts", self._lib.nb_pair_counts(self._h, e.ctypes.data, e.size - 1, counts.ctypes.data), self._lib)
        return counts

    def radial_profiles(self, centers, edges, vcenters=None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Shell sums about many centres, reduced on the device (``nb_radial_profiles``; synchronises).  ``centers`` is
        ``(ncenters, dims)``, passed on as float32; ``edges`` the ``nbins + 1`` strictly ascending shell edges, 1 <= nbins <= 64, passed
        on as float32; ``vcenters`` the centres' velocities, ``(ncenters, dims)``, passed on as float64 (default: zero).  Returns a
        ``(ncenters, nbins)`` ``SHELL_DTYPE`` array: ``count`` and the fp64 sums ``mass``, ``mr``, ``mr2``, ``mvr``, ``mvr2``, ``mv2``,
        ``mlz`` of the bodies with ``edges[b]**2 <= d2 < edges[b+1]**2`` about centre c, d2 in fp32 (3-D on a ``dims = 3`` handle).
        ``out``: a writeable C-contiguous ``SHELL_DTYPE`` array of that shape (one over ``nb_host_alloc`` memory is written by the copy
        engine directly); default a new array.  The handle must own all n bodies.  The arguments are validated by the library
        (include/nbody.h has the rules)."""
        dims = 3 if self._params.dims == 3 else 2
        c = np.ascontiguousarray(centers, dtype=np.float32)
        if c.ndim != 2 or c.shape[1] != dims:
            raise ValueError(f"radial_profiles: centers must be (ncenters, {dims}) (got shape {c.shape})")
        e = np.ascontiguousarray(edges, dtype=np.float32)
        if e.ndim != 1 or e.size < 2:
            raise ValueError("radial_profiles: edges must be a 1-D sequence of at least two values")
        v = None
        if vcenters is not None:
            v = np.ascontiguousarray(vcenters, dtype=np.float64)
            if v.shape != c.shape:
                raise ValueError(f"radial_profiles: vcenters must have the shape of centers, {c.shape} (got {v.shape})")
        shape = (c.shape[0], e.size - 1)
        if out is None:
            out = np.zeros(shape, dtype=L.SHELL_DTYPE)
        elif (not isinstance(out, np.ndarray) or out.dtype != L.SHELL_DTYPE or out.shape != shape or not out.flags.c_contiguous
              or not out.flags.writeable):
            raise TypeError(f"out must be a writeable C-contiguous {shape} numpy array of nbodysim_amd.SHELL_DTYPE (64-byte nb_shell records)")
        L.check("nb_radial_profiles", self._lib.nb_radial_profiles(self._h, c.ctypes.data, None if v is None else v.ctypes.data, c.shape[0],
                                                                   e.ctypes.data, e.size - 1, out.ctypes.data), self._lib)
        return out

    def field(self, points, phi: bool = True, acc: bool = True, out=None):
        """Potential and acceleration of all n bodies at arbitrary points (``nb_field``; synchronises).  ``points`` is
        ``(npoints, dims)``, passed on as float32.  Returns ``phi`` (float64, ``(npoints,)``), ``acc`` (float64, ``(npoints, dims)``) or
        the pair ``(phi, acc)``, as asked for; a plane that is not asked for is not computed.  ``out``: the destination, a writeable
        C-contiguous float64 array of that shape, or the pair of them where both planes are asked for (one over ``nb_host_alloc``
        memory is written by the copy engine directly); default new arrays.  A point is not a body: no self term; a point on a body
        takes ``-m / eps`` into phi and nothing into acc.  The arguments are validated by the library (include/nbody.h has the rules)."""
        if not (phi or acc):
            raise ValueError("field: at least one of phi and acc must be asked for")
        dims = 3 if self._params.dims == 3 else 2
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != dims:
            raise ValueError(f"field: points must be (npoints, {dims}) (got shape {p.shape})")
        want = ([("phi", (p.shape[0],))] if phi else []) + ([("acc", (p.shape[0], dims))] if acc else [])
        if out is None:
            planes = [np.empty(shape, dtype=np.float64) for _, shape in want]
        else:
            planes = list(out) if len(want) == 2 and isinstance(out, (tuple, list)) else [out]
            if len(planes) != len(want):
                raise TypeError("out must be a pair (phi, acc) of arrays where both planes are asked for, one array otherwise")
            for a, (what, shape) in zip(planes, want):
                if (not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.shape != shape or not a.flags.c_contiguous
                        or not a.flags.writeable):
                    raise TypeError(f"out for {what} must be a writeable C-contiguous {shape} numpy array of float64")
        by = dict(zip((w for w, _ in want), planes))
        L.check("nb_field", self._lib.nb_field(self._h, p.ctypes.data, p.shape[0], by["phi"].ctypes.data if phi else None,
                                               by["acc"].ctypes.data if acc else None), self._lib)
        return tuple(planes) if len(planes) == 2 else planes[0]

    def jerks(self, acc: bool = True, jerk: bool = True):
        """Acceleration and jerk (its time derivative) of every body at the current positions and velocities (``nb_jerks``;
        ``integrator="hermite4"`` handles only; synchronises; changes nothing of the handle).  Returns ``acc`` or ``jerk`` (float64,
        ``(n, dims)``) or the pair ``(acc, jerk)``, as asked for."""
        if not (acc or jerk):
            raise ValueError("jerks: at least one of acc and jerk must be asked for")
        dims = 3 if self._params.dims == 3 else 2
        planes = [np.empty((self.n, dims), dtype=np.float64) if want else None for want in (acc, jerk)]
        L.check("nb_jerks", self._lib.nb_jerks(self._h, *(None if a is None else a.ctypes.data for a in planes)), self._lib)
        got = [a for a in planes if a is not None]
        return tuple(got) if len(got) == 2 else got[0]

    def set_tree_alpha(self, alpha: float) -> None:
        """Set alpha of the acceleration-relative opening test (``nb_tree_alpha``; ``tree_alpha`` handles only) between steps."""
        L.check("nb_tree_alpha", self._lib.nb_tree_alpha(self._h, alpha), self._lib)

    def body_order(self, every: int = 0, perm: bool = False):
        """The body order of the handle (``nb_body_order``): returns the force evaluations from one sort to the next (0: the handle
        sweeps its bodies in the caller's order); ``every`` > 0 sets that cadence first; with ``perm`` returns ``(every, perm)``, perm
        the uint32 permutation of the last sort (sorted position -> body index; synchronises)."""
        out = np.empty(self.n, dtype=np.uint32) if perm else None
        ev = C.c_uint32(0)
        L.check("nb_body_order", self._lib.nb_body_order(self._h, every, out.ctypes.data if perm else None, C.byref(ev)), self._lib)
        return (int(ev.value), out) if perm else int(ev.value)

    def dump(self, path: str) -> None:
        L.check("nb_dump", self._lib.nb_dump(self._h, str(path).encode()), self._lib)

    # split step for sharded handles
    def step_begin(self, dt: Optional[float] = None) -> None:
        L.check("nb_step_begin", self._lib.nb_step_begin(self._h, SIMULATION_DT if dt is None else dt), self._lib)

    def step_mid(self) -> None:
        L.check("nb_step_mid", self._lib.nb_step_mid(self._h), self._lib)

    def step_finish(self) -> None:
        L.check("nb_step_finish", self._lib.nb_step_finish(self._h), self._lib)

    def pos_buffer(self, which: int = L.NB_POS_CURRENT) -> int:
        return int(self._lib.nb_pos_buffer(self._h, which) or 0)

    @property
    def shard_protocol(self) -> int:
        return int(self._lib.nb_shard_protocol(self._h))

    def acc_buffer(self, which: int) -> int:
        return int(self._lib.nb_acc_buffer(self._h, which) or 0)

    @property
    def stream(self) -> int:
        return int(self._lib.nb_stream(self._h) or 0)

    def profile(self, on: bool = True) -> None:
        L.check("nb_profile_enable", self._lib.nb_profile_enable(self._h, int(on)), self._lib)

    def profile_read(self, reset: bool = True) -> tuple:
        ms, cnt = C.c_double(), C.c_uint64()
        L.check("nb_profile_read", self._lib.nb_profile_read(self._h, C.byref(ms), C.byref(cnt), int(reset)), self._lib)
        return ms.value, int(cnt.value)

    def sym_info(self) -> dict:
        """Figures of the symmetric work plan (``nb_sym_plan_info``): items, chunks per item, slab bytes ..."""
        info = L.nb_sym_info()
        info.struct_size = C.sizeof(L.nb_sym_info)
        L.check("nb_sym_plan_info", self._lib.nb_sym_plan_info(self._h, C.byref(info)), self._lib)
        return info.as_dict()

    def describe(self) -> str:
        buf = C.create_string_buffer(2048)
        L.check("nb_describe", self._lib.nb_describe(self._h, buf, len(buf)), self._lib)
        return buf.value.decode()

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.nb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_bodies(path: str, bodies: np.ndarray, frame: int = 0, eps: float = 1.0, dt: float = SIMULATION_DT) -> None:
    p = L.default_params()
    p.eps, p.dt = eps, dt
    bodies = np.ascontiguousarray(bodies)
    L.check("nb_write_bodies", L.load().nb_write_bodies(str(path).encode(), bodies.ctypes.data, bodies.shape[0], frame, C.byref(p)))


def read_bodies(path: str):
    """Return (bodies, frame, params) of a dump written by nb_dump / nb_write_bodies."""
    lib = L.load()
    n, frame, p = C.c_size_t(), C.c_uint64(), L.nb_params()
    L.check("nb_read_header", lib.nb_read_header(str(path).encode(), C.byref(n), C.byref(frame), C.byref(p)))
    out = L.bodies_array(n.value)
    L.check("nb_read_bodies", lib.nb_read_bodies(str(path).encode(), out.ctypes.data, n.value))
    return out, int(frame.value), p
