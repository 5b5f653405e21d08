"""Host-side mirror of the reference's FEM class surface over the C ABI.

``FemIntegrator`` plays the role of ``VolumeConservingIntegrator`` + ``CorotationalLinearFEMForceModel``
(reference src/deformable/PS_VolumeConservingIntegrator.{h,cpp}, vegafem/integrator/integratorBase*.h): same
method names in snake_case, same argument meaning, same error behaviour except that a failed solve raises
``FbError(FB_ESOLVER)`` instead of ``exit(-1)``.  ``Deformable`` mirrors the per-step driver of
``Deformable::timestep`` (reference src/deformable/Deformable.cpp:318-420).
"""
import ctypes as C

import numpy as np

from . import lib as _l
from .meshgen import fixed_vertices_to_dofs


class FemIntegrator:
    def __init__(self, verts, tets, fixed_dofs=(), E=1e7, nu=0.46, rho=1000.0, timestep=0.0333,
                 damping_mass=0.0, damping_stiffness=0.01, cg_eps=1e-6, cg_max_iter=10000,
                 matrix_precision=_l.FB_MATRIX_AUTO, device=0, shard=None, pcg_variant=_l.FB_PCG_MERGED, spmv_kernel=_l.FB_SPMV_AUTO,
                 linear=False, exact_tangent=False, integrator=_l.FB_INTEGRATOR_VOLUME_CONSERVING, renumber=_l.FB_RENUMBER_AUTO, expect_cuts=False,
                 reserve_nodes=0, reserve_elements=0):
        """shard = (n_ranks, rank, node_splits or None, comm_handle) for a domain-decomposed handle."""
        L = _l.lib()
        self._L = L
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.tets = np.ascontiguousarray(tets, dtype=np.int32).reshape(-1, 4)
        self.n_nodes, self.n_tets_global = len(self.verts), len(self.tets)
        self.r = 3 * self.n_nodes
        fd = _l.as_i32(fixed_dofs)
        p = _l.FemParams()
        L.fb_fem_default_params(C.byref(p))
        p.E, p.nu, p.rho, p.timestep = E, nu, rho, timestep
        p.damping_mass, p.damping_stiffness = damping_mass, damping_stiffness
        p.cg_eps, p.cg_max_iter, p.matrix_precision, p.device = cg_eps, cg_max_iter, matrix_precision, device
        p.pcg_variant = pcg_variant
        p.spmv_kernel = spmv_kernel
        p.linear = 1 if linear else 0
        p.exact_tangent = 1 if exact_tangent else 0
        p.integrator = integrator
        p.renumber = renumber
        p.expect_cuts, p.reserve_nodes, p.reserve_elements = int(bool(expect_cuts)), int(reserve_nodes), int(reserve_elements)
        self.params = p
        self.h = C.c_void_p()
        self.node_lo, self.node_hi = 0, self.n_nodes
        if shard is None:
            _l.check(L.fb_fem_create(C.byref(self.h), self.n_nodes, _l.dptr(self.verts), self.n_tets_global,
                                     _l.iptr(self.tets), len(fd), _l.iptr(fd), C.byref(p)))
        else:
            n_ranks, rank, splits, comm = shard
            sp = None if splits is None else _l.as_i32(splits)
            _l.check(L.fb_fem_create_sharded(C.byref(self.h), self.n_nodes, _l.dptr(self.verts), self.n_tets_global,
                                             _l.iptr(self.tets), len(fd), _l.iptr(fd), C.byref(p), n_ranks, rank,
                                             _l.iptr(sp), comm))
            if sp is None:
                sp = np.array([self.n_nodes * i // n_ranks for i in range(n_ranks + 1)], dtype=np.int32)
            self.node_lo, self.node_hi = int(sp[rank]), int(sp[rank + 1])
        self.last = _l.StepInfo()
        self._embed_n = {}  # points of every live embedding, by id

    @classmethod
    def from_poly(cls, poly, fixed_dofs=(), E=1e7, nu=0.46, rho=1000.0, timestep=0.0333, damping_mass=0.0, damping_stiffness=0.01,
                  cg_eps=1e-6, cg_max_iter=10000, matrix_precision=_l.FB_MATRIX_AUTO, device=0, linear=False):
        """The tet mesh a GpuPoly holds on the device (after tetrahedralize) as the FEM mesh, without a host copy
        (fb_fem_create_from_poly).  verts / tets are read back only for the Python-side conveniences."""
        self = cls.__new__(cls)
        L = _l.lib()
        self._L = L
        xyz, tets = poly.read_tetmesh()
        self.verts = xyz.astype(np.float64)
        self.tets = tets.astype(np.int32)
        self.n_nodes, self.n_tets_global = len(self.verts), len(self.tets)
        self.r = 3 * self.n_nodes
        fd = _l.as_i32(fixed_dofs)
        p = _l.FemParams()
        L.fb_fem_default_params(C.byref(p))
        p.E, p.nu, p.rho, p.timestep = E, nu, rho, timestep
        p.damping_mass, p.damping_stiffness = damping_mass, damping_stiffness
        p.cg_eps, p.cg_max_iter, p.matrix_precision, p.device = cg_eps, cg_max_iter, matrix_precision, device
        p.linear = 1 if linear else 0
        self.params = p
        self.h = C.c_void_p()
        self.node_lo, self.node_hi = 0, self.n_nodes
        _l.check(L.fb_fem_create_from_poly(C.byref(self.h), poly.h, len(fd), _l.iptr(fd), C.byref(p)))
        self.last = _l.StepInfo()
        self._embed_n = {}  # points of every live embedding, by id
        return self

    # -- life cycle --
    def time_element_stiffness(self, reps=5):
        """Seconds to form K0 = V B^T E B of every element with the fp64 MFMA kernel (inspection path)."""
        a = C.c_double(0)
        _l.check(self._L.fb_fem_time_element_stiffness(self.h, reps, C.byref(a)))
        return a.value

    def time_exchange(self, reps=100):
        """(seconds per halo refresh, seconds per 3-scalar global sum); collective on a sharded handle."""
        a, b = C.c_double(0), C.c_double(0)
        _l.check(self._L.fb_fem_time_exchange(self.h, reps, C.byref(a), C.byref(b)))
        return a.value, b.value

    def transport(self):
        """0 unsharded, else the exchange mode in use (lib.FB_XCH_*)."""
        return int(self._L.fb_fem_transport(self.h))

    def set_exchange_mode(self, mode):
        """Collective: every rank of a sharded handle switches between two solves."""
        _l.check(self._L.fb_fem_set_exchange_mode(self.h, mode))

    def renumbering(self):
        """(works in an internal node order?, widest element in the caller's order, in the internal order)"""
        a, b = C.c_int(0), C.c_int(0)
        on = self._L.fb_fem_renumbering(self.h, C.byref(a), C.byref(b))
        return bool(on), a.value, b.value

    def owned_nodes(self):
        """caller ids of the owned nodes in internal order"""
        ids = np.empty(self.node_hi - self.node_lo, np.int32)
        _l.check(self._L.fb_fem_owned_nodes(self.h, _l.iptr(ids)))
        return ids

    def halo_info(self):
        """(halo nodes, neighbour ranks) of a sharded handle"""
        a, b = C.c_int(0), C.c_int(0)
        _l.check(self._L.fb_fem_halo_info(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sharded_persist(self):
        """True when this sharded handle's solves run inside the sharded persistent launches (FEMBRAIN_SHARDED_PERSIST=1)."""
        return bool(self._L.fb_fem_sharded_persist(self.h))

    def set_sharded_persist(self, on):
        """Collective: every rank switches between two solves."""
        _l.check(self._L.fb_fem_set_sharded_persist(self.h, 1 if on else 0))

    def close(self):
        if getattr(self, "h", None):
            self._L.fb_fem_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resync(self, verts, tets, fixed_dofs=(), node_splits=None):
        """Deformable::syncForceModel after a cut.  On a sharded handle the call is collective; node_splits = the new node
        ranges (None: kept when the node count is unchanged, else the equal split)."""
        self.verts = np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)
        self.tets = np.ascontiguousarray(tets, dtype=np.int32).reshape(-1, 4)
        self.n_nodes, self.r = len(self.verts), 3 * len(self.verts)
        fd = _l.as_i32(fixed_dofs)
        sp = None if node_splits is None else _l.as_i32(node_splits)
        _l.check(self._L.fb_fem_resync_sharded(self.h, self.n_nodes, _l.dptr(self.verts), len(self.tets), _l.iptr(self.tets),
                                               len(fd), _l.iptr(fd), _l.iptr(sp)))
        rng = (C.c_int * 2)()
        _l.check(self._L.fb_fem_owned_range(self.h, rng))
        self.node_lo, self.node_hi = int(rng[0]), int(rng[1])

    def resync_delta(self, delta, fixed_dofs=(), track=True):
        """The same from a description of the change (fb_fem_resync_delta): delta = dict(removed, changed_ids, changed_nodes, added,
        new_xyz) in the terms of ``meshgen.apply_delta`` -- ids of the handle's current element list, new nodes appended.  The
        mesh stays on the device; ``self.verts`` / ``self.tets`` follow on the host for the caller's convenience (track=False: they
        are dropped instead -- timing runs)."""
        from .meshgen import apply_delta
        rem = _l.as_i32(delta.get("removed", ()))
        cid = _l.as_i32(delta.get("changed_ids", ()))
        cno = np.ascontiguousarray(delta.get("changed_nodes", ()), dtype=np.int32).reshape(-1)
        add = np.ascontiguousarray(delta.get("added", ()), dtype=np.int32).reshape(-1)
        nxy = np.ascontiguousarray(delta.get("new_xyz", ()), dtype=np.float64).reshape(-1)
        fd = _l.as_i32(fixed_dofs)
        _l.check(self._L.fb_fem_resync_delta(self.h, len(rem), _l.iptr(rem), len(cid), _l.iptr(cid), _l.iptr(cno), len(add) // 4, _l.iptr(add),
                                             len(nxy) // 3, _l.dptr(nxy), len(fd), _l.iptr(fd)))
        if track and self.verts is not None:
            self.verts, self.tets = apply_delta(self.verts, self.tets, dict(removed=rem, changed_ids=cid, changed_nodes=cno, added=add, new_xyz=nxy))
            self.n_nodes = len(self.verts)
        else:
            self.verts = self.tets = None
            self.n_nodes = int(self._L.fb_fem_num_nodes(self.h))
        self.r = 3 * self.n_nodes
        self.node_lo, self.node_hi = 0, self.n_nodes

    def cut(self, strip, mode="bake", modify=True, track=True):
        """CuttableMesh::cut + Deformable::syncForceModel in one device call (fb_fem_cut): ``strip`` is the blade's swept quad strip
        ((2m, 3) points, quad i = points 2i .. 2i+3).  mode "bake" (FemBrain: the deformed shape becomes the rest shape, state reset) or
        "carry" (rest shape and state kept, new nodes interpolated).  Returns (info, delta): info a dict of the fb_cut_result fields,
        delta the change in ``meshgen.apply_delta``'s terms (removed, changed_ids, changed_nodes, added, new_xyz) plus per new node
        its cut edge (edge_nodes, lo and hi caller ids) and fraction (edge_frac), and the first unhandled element ids / codes.  The
        delta is empty unless the status is FB_CUT_DONE or FB_CUT_DRY.  With track, ``self.verts`` / ``self.tets`` follow the cut."""
        modes = {"bake": _l.FB_CUT_BAKE, "carry": _l.FB_CUT_CARRY}
        if mode not in modes:
            raise ValueError("mode is 'bake' or 'carry', not %r" % (mode,))
        pts = np.ascontiguousarray(strip, dtype=np.float64).reshape(-1)
        if pts.size % 3:
            raise ValueError("strip points are xyz triples")
        res = _l.CutResult()
        _l.check(self._L.fb_fem_cut(self.h, pts.size // 3, _l.dptr(pts), modes[mode], 1 if modify else 0, C.byref(res)))
        info = {name: getattr(res, name) for name, _ in _l.CutResult._fields_}
        nr, na, nn = res.n_removed, res.n_added, res.n_new_nodes
        nu = min(res.n_unhandled, _l.FB_CUT_UNHANDLED_IDS)
        removed, added = np.zeros(nr, np.int32), np.zeros((na, 4), np.int32)
        new_xyz, edge_nodes, edge_frac = np.zeros((nn, 3)), np.zeros((nn, 2), np.int32), np.zeros(nn)
        uid, ucode = np.zeros(nu, np.int32), np.zeros(nu, np.int32)
        _l.check(self._L.fb_fem_read_cut(self.h, _l.iptr(removed), _l.iptr(added), _l.dptr(new_xyz), _l.iptr(edge_nodes), _l.dptr(edge_frac),
                                         _l.iptr(uid), _l.iptr(ucode)))
        delta = dict(removed=removed, changed_ids=np.zeros(0, np.int32), changed_nodes=np.zeros((0, 4), np.int32), added=added, new_xyz=new_xyz,
                     edge_nodes=edge_nodes, edge_frac=edge_frac, unhandled_ids=uid, unhandled_codes=ucode)
        if res.status == _l.FB_CUT_DONE:
            self.n_nodes = int(self._L.fb_fem_num_nodes(self.h))
            self.r = 3 * self.n_nodes
            self.node_lo, self.node_hi = 0, self.n_nodes
            if track:
                self.verts, self.tets = self.read_mesh()
        return info, delta

    def read_mesh(self):
        """(rest positions (n, 3), elements (m, 4)) as the device holds them, in the caller's numbering (fb_fem_read_mesh)"""
        n, m = int(self._L.fb_fem_num_nodes(self.h)), int(self._L.fb_fem_num_tets(self.h))
        xyz, tets = np.zeros((n, 3)), np.zeros((m, 4), np.int32)
        _l.check(self._L.fb_fem_read_mesh(self.h, _l.dptr(xyz), _l.iptr(tets)))
        return xyz, tets

    def surface(self):
        """The boundary triangles of the mesh the device holds (fb_fem_surface; SurfaceMesh::setupFromTetMesh): dict of faces (F, 3) and
        face_tets (F,) in the caller's numbering, vertex_ids (V,) the ascending ids of the nodes on the surface, n_builds, and aabb
        (2, 3) of the surface's rest positions.  Built on the device, and again only after the mesh has changed."""
        info = _l.SurfaceInfo()
        _l.check(self._L.fb_fem_surface(self.h, C.byref(info)))
        faces, vids, ft = np.zeros((info.n_faces, 3), np.int32), np.zeros(info.n_vertices, np.int32), np.zeros(info.n_faces, np.int32)
        _l.check(self._L.fb_fem_read_surface(self.h, _l.iptr(faces), _l.iptr(vids), _l.iptr(ft)))
        return dict(faces=faces, vertex_ids=vids, face_tets=ft, n_builds=int(info.n_builds),
                    aabb=np.array([list(info.aabb_lo), list(info.aabb_hi)], np.float32))

    def surface_update(self):
        """(xyz (V, 3) float32, normals (V, 3) float32, aabb (2, 3) float32) of the surface vertices at the current state, in
        ``surface()['vertex_ids']`` order (fb_fem_surface_update; SurfaceMesh::applyDisplacements, VolMeshRender::sync)"""
        info = _l.SurfaceInfo()
        _l.check(self._L.fb_fem_surface(self.h, C.byref(info)))
        xyz, nrm = np.zeros((info.n_vertices, 3), np.float32), np.zeros((info.n_vertices, 3), np.float32)
        _l.check(self._L.fb_fem_surface_update(self.h, _l.fptr(xyz), _l.fptr(nrm), C.byref(info)))
        return xyz, nrm, np.array([list(info.aabb_lo), list(info.aabb_hi)], np.float32)

    def time_surface(self, reps=20):
        """(seconds per build, seconds per update): medians of ``reps`` HIP-event timings each (fb_fem_time_surface)"""
        b, u = C.c_double(0), C.c_double(0)
        _l.check(self._L.fb_fem_time_surface(self.h, reps, C.byref(b), C.byref(u)))
        return b.value, u.value

    # -- embedded point sets: the drawn mesh bound to the tets and moved on the device (fb_fem_embed; unsharded handles) --
    @staticmethod
    def _embed_info(info):
        return dict(id=int(info.id), n_points=int(info.n_points), n_triangles=int(info.n_triangles), n_external=int(info.n_external),
                    n_zeroed=int(info.n_zeroed), n_locates=int(info.n_locates), n_rebound=int(info.n_rebound), grid=tuple(info.grid),
                    n_wide=int(info.n_wide), aabb=np.array([list(info.aabb_lo), list(info.aabb_hi)], np.float32))

    def _embed_points(self, eid):
        if eid not in self._embed_n:
            _l.check(self._L.fb_fem_read_embedding(self.h, int(eid), None, None, None, None))  # (the library's refusal and its text)
            raise ValueError("no embedding %r was made through this object" % (eid,))
        return self._embed_n[eid]

    def embed(self, points, triangles=None, zero_threshold=0.0, info=False):
        """Bind ``points`` (n, 3) in the rest frame, optionally with ``triangles`` (m, 3) over them, to the elements of the mesh the
        device holds (fb_fem_embed; VolumetricMesh::generateInterpolationWeights): the id of the embedding, with ``info`` also the
        dict of counts (n_external, n_zeroed, grid, n_wide, ...) and the box of the bound points in the rest shape."""
        pts = _l.as_f64(points)
        if pts.size % 3:
            raise ValueError("points: (n, 3)")
        tri = None if triangles is None else _l.as_i32(triangles)
        if tri is not None and tri.size % 3:
            raise ValueError("triangles: (m, 3)")
        prm = _l.EmbedParams(float(zero_threshold))
        eid, out = C.c_int(-1), _l.EmbedInfo()
        _l.check(self._L.fb_fem_embed(self.h, pts.size // 3, _l.dptr(pts), 0 if tri is None else tri.size // 3, _l.iptr(tri),
                                      C.byref(prm), C.byref(eid), C.byref(out)))
        self._embed_n[eid.value] = pts.size // 3  # (point count per id: sizes of the read-backs)
        return (eid.value, self._embed_info(out)) if info else eid.value

    def embed_from_poly(self, poly, zero_threshold=0.0, info=False):
        """The current marching-cubes surface of a GpuPoly (after ``surface()``) as an embedding, handed over on the device
        (fb_fem_embed_from_poly): the same as ``embed(*poly.read_surface()[::2])`` without the host copy"""
        prm = _l.EmbedParams(float(zero_threshold))
        eid, out = C.c_int(-1), _l.EmbedInfo()
        _l.check(self._L.fb_fem_embed_from_poly(self.h, poly.h, C.byref(prm), C.byref(eid), C.byref(out)))
        self._embed_n[eid.value] = int(out.n_points)
        return (eid.value, self._embed_info(out)) if info else eid.value

    def embedding(self, eid):
        """dict of elements (n,), vertices (n, 4) in the caller's numbering, weights (n, 4) and rest_xyz (n, 3) of embedding ``eid``
        (fb_fem_read_embedding); after a fb_fem_resync the points are searched again first"""
        n = self._embed_points(eid)
        el, vt, w, xyz = np.zeros(n, np.int32), np.zeros((n, 4), np.int32), np.zeros((n, 4)), np.zeros((n, 3))
        _l.check(self._L.fb_fem_read_embedding(self.h, eid, _l.iptr(el), _l.iptr(vt), _l.dptr(w), _l.dptr(xyz)))
        return dict(elements=el, vertices=vt, weights=w, rest_xyz=xyz)

    def embed_update(self, eid, positions=True, normals=True):
        """(xyz (n, 3) float32, normals (n, 3) float32, info dict) of the embedded points at the current state (fb_fem_embed_update);
        ``positions`` / ``normals`` False: that array is not copied out (None)"""
        n = self._embed_points(eid)
        xyz = np.zeros((n, 3), np.float32) if positions else None
        nrm = np.zeros((n, 3), np.float32) if normals else None
        out = _l.EmbedInfo()
        _l.check(self._L.fb_fem_embed_update(self.h, eid, _l.fptr(xyz), _l.fptr(nrm), C.byref(out)))
        return xyz, nrm, self._embed_info(out)

    def embed_release(self, eid):
        _l.check(self._L.fb_fem_embed_release(self.h, eid))
        self._embed_n.pop(eid, None)

    # -- the way back from an embedding: forces on drawn points, picks, stress per point (fb_fem_embed_add_forces / pick_ray / ...) --
    def embed_add_forces(self, eid, forces, point_ids=None):
        """The transpose of embedding ``eid``, added into the current external force vector (fb_fem_embed_add_forces): ``forces[s]``
        on point ``point_ids[s]`` (strictly ascending; None: ``forces`` (n_points, 3) on every point) goes to the four nodes of the
        point's element by its weights -- bit for bit ``for p, k, c: fext[3 v + c] += w[p, k] * f[p, c]`` over ``embedding(eid)``."""
        n_points = self._embed_points(eid)
        ids = None if point_ids is None else _l.as_i32(point_ids)
        n = n_points if ids is None else len(ids)
        f = _l.as_f64(forces, 3 * n)
        _l.check(self._L.fb_fem_embed_add_forces(self.h, int(eid), n, _l.iptr(ids), _l.dptr(f)))

    def embed_forces_info(self, eid):
        """dict of n_table_builds (transposed tables built for embedding ``eid``), longest_run (most corners of one node) and
        n_nodes_touched (nodes with a corner) of the last one (fb_fem_embed_forces_info)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        _l.check(self._L.fb_fem_embed_forces_info(self.h, int(eid), C.byref(a), C.byref(b), C.byref(c)))
        return dict(n_table_builds=a.value, longest_run=b.value, n_nodes_touched=c.value)

    def embed_pick_ray(self, eid, origin, direction, t_max=np.inf):
        """The nearest hit of the ray ``origin + t direction``, 0 <= t <= t_max, on the triangles of embedding ``eid`` at the current
        state (fb_fem_embed_pick_ray): dict of triangle (-1: a miss), t, bary (u, v) -- the hit is (1-u-v) a + u b + v c -- and xyz"""
        self._embed_points(eid)
        o, d = _l.as_f64(origin, 3), _l.as_f64(direction, 3)
        tri, t, bary, xyz = C.c_int(-1), C.c_double(0), np.zeros(2), np.zeros(3)
        _l.check(self._L.fb_fem_embed_pick_ray(self.h, int(eid), _l.dptr(o), _l.dptr(d), float(t_max), C.byref(tri), C.byref(t), _l.dptr(bary), _l.dptr(xyz)))
        return dict(triangle=tri.value, t=t.value, bary=bary, xyz=xyz)

    def embed_pick_point(self, eid, wpos):
        """(index, position (3,), squared distance) of the point of embedding ``eid`` closest to ``wpos`` at the current state; of
        equal distances the lowest id (fb_fem_embed_pick_point)"""
        self._embed_points(eid)
        w = _l.as_f64(wpos, 3)
        idx, xyz, d2 = C.c_int(-1), np.zeros(3), C.c_double(0)
        _l.check(self._L.fb_fem_embed_pick_point(self.h, int(eid), _l.dptr(w), C.byref(idx), _l.dptr(xyz), C.byref(d2)))
        return idx.value, xyz, d2.value

    def embed_stress(self, eid):
        """(n_points,) float32: the von Mises stress of the element each point of embedding ``eid`` is bound to, from the last
        ``stress()`` (fb_fem_embed_stress) -- the colour to draw on ``embed_update()``'s points"""
        n = self._embed_points(eid)
        vm = np.zeros(n, np.float32)
        _l.check(self._L.fb_fem_embed_stress(self.h, int(eid), _l.fptr(vm)))
        return vm

    def time_embed(self, eid, reps=20):
        """(seconds per full search, seconds per update): medians of ``reps`` HIP-event timings each (fb_fem_time_embed)"""
        a, b = C.c_double(0), C.c_double(0)
        _l.check(self._L.fb_fem_time_embed(self.h, eid, reps, C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_embed_search(self, eid, reps=20):
        """(grid build, search through the grid, external pass with weights and counts): seconds, medians of ``reps`` (fb_fem_time_embed_search)"""
        out = np.zeros(3)
        _l.check(self._L.fb_fem_time_embed_search(self.h, eid, reps, _l.dptr(out)))
        return tuple(float(x) for x in out)

    def embed_search_info(self, eid):
        """What the pass for the points no element contains did in the last search of embedding ``eid`` (fb_fem_embed_search_info_get):
        dict of path (lib.FB_EMBED_CLOSEST_NONE / _SCAN / _RING), n_outside, n_far (the points the full scan finished),
        centre_grid_builds (of the handle), max_centres_one_point and centres_tested"""
        out = _l.EmbedSearchInfo()
        _l.check(self._L.fb_fem_embed_search_info_get(self.h, int(eid), C.byref(out)))
        return {name: int(getattr(out, name)) for name, _ in _l.EmbedSearchInfo._fields_}

    def time_embed_closest(self, eid, path, reps=20):
        """(centre-grid build, external pass) in seconds for the outside points of embedding ``eid`` with ``path``
        (lib.FB_EMBED_CLOSEST_SCAN or _RING), medians of ``reps``, on a scratch copy (fb_fem_time_embed_closest)"""
        out = np.zeros(2)
        _l.check(self._L.fb_fem_time_embed_closest(self.h, int(eid), int(reps), int(path), _l.dptr(out)))
        return float(out[0]), float(out[1])

    # -- disjoint parts of the (cut) mesh on the device (fb_fem_parts / split_parts / read_part; unsharded handles) --
    def parts(self):
        """The face-connected parts of the mesh the device holds (fb_fem_parts; VolMesh::get_disjoint_parts): dict of n_parts,
        n_builds, largest_part, n_shared_nodes (nodes of more than one part) and n_unused_nodes.  Labelled on the device, and again
        only after the mesh has changed."""
        info = _l.PartsInfo()
        _l.check(self._L.fb_fem_parts(self.h, C.byref(info)))
        return {name: getattr(info, name) for name, _ in _l.PartsInfo._fields_}

    def element_parts(self):
        """(n_tets,) int32: the part of every element, ``read_mesh``'s element order; parts ascend with their smallest element"""
        out = np.zeros(int(self._L.fb_fem_num_tets(self.h)), np.int32)
        _l.check(self._L.fb_fem_read_parts(self.h, _l.iptr(out), None, None, None, None, None))
        return out

    def node_parts(self):
        """(n_nodes,) int32: the lowest part whose elements use the node (caller ids), -1 for a node no element uses"""
        out = np.zeros(int(self._L.fb_fem_num_nodes(self.h)), np.int32)
        _l.check(self._L.fb_fem_read_parts(self.h, None, _l.iptr(out), None, None, None, None))
        return out

    def part_table(self):
        """Per part: dict of elements, nodes (a shared node counts in each of its parts), first_element (n_parts,) int32 and volume
        (n_parts,) float64, the rest volume of the part's elements summed in a fixed order"""
        n = self.parts()["n_parts"]
        el, nd, fe, vol = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
        _l.check(self._L.fb_fem_read_parts(self.h, None, None, _l.iptr(el), _l.iptr(nd), _l.iptr(fe), _l.dptr(vol)))
        return dict(elements=el, nodes=nd, first_element=fe, volume=vol)

    def split_parts(self, quad, dist, track=True):
        """``CuttableMesh::splitParts(sweptquad, dist)`` on the rest positions (fb_fem_split_parts): the parts wholly in front of the
        quad's plane move by +shift, those wholly behind by -shift, straddling parts stay.  Returns the dict of n_front_parts,
        n_back_parts, n_straddling_parts, n_nodes_moved and shift (3,).  With track, ``self.verts`` follows."""
        qd = np.ascontiguousarray(quad, dtype=np.float64).reshape(-1)
        if qd.size != 12:
            raise ValueError("a quad is four xyz points")
        info = _l.SplitInfo()
        _l.check(self._L.fb_fem_split_parts(self.h, _l.dptr(qd), float(dist), C.byref(info)))
        if track:
            self.verts = self.read_mesh()[0]
        return dict(n_front_parts=int(info.n_front_parts), n_back_parts=int(info.n_back_parts), n_straddling_parts=int(info.n_straddling_parts),
                    n_nodes_moved=int(info.n_nodes_moved), shift=np.array(list(info.shift)))

    def read_part(self, k):
        """Part ``k`` as a mesh of its own (fb_fem_read_part; one iteration of ``convertDisjointPartsToMeshes``): (element_ids (m,),
        node_ids (n,) caller ids in order of first use, rest_xyz (n, 3), tets_local (m, 4)) -- what a second ``FemIntegrator`` is made of"""
        n = self.parts()["n_parts"]
        if not 0 <= int(k) < n:
            _l.check(self._L.fb_fem_read_part(self.h, int(k), None, None, None, None))
        t = self.part_table()
        m, nn = int(t["elements"][k]), int(t["nodes"][k])
        ids, nodes, xyz, tl = np.zeros(m, np.int32), np.zeros(nn, np.int32), np.zeros((nn, 3)), np.zeros((m, 4), np.int32)
        _l.check(self._L.fb_fem_read_part(self.h, int(k), _l.iptr(ids), _l.iptr(nodes), _l.dptr(xyz), _l.iptr(tl)))
        return ids, nodes, xyz, tl

    def detach_part(self, k, remove=False, track=True):
        """Part ``k`` as a ``FemIntegrator`` of its own, made on the device (fb_fem_detach_part; ``convertDisjointPartsToMeshes``): the
        piece's mesh is ``read_part(k)``'s, and it takes over this handle's parameters, the state and external forces of its nodes, its
        elements' materials and the constrained DOFs on its nodes.  ``remove`` erases the part's elements from this handle (state and
        forces carried, node count unchanged; ``self.tets`` follows).  Returns (piece, element_ids, node_ids); ``piece.detach_info`` is
        the dict of the fb_fem_detach_info fields.  With track, ``piece.verts`` / ``piece.tets`` are read back for the caller's
        convenience (track=False: nothing but the two id arrays leaves the device -- timing runs)."""
        n = self.parts()["n_parts"]
        flags = _l.FB_DETACH_REMOVE if remove else _l.FB_DETACH_KEEP
        out = C.c_void_p()
        if not 0 <= int(k) < n or (remove and n < 2):  # (refused: nothing to size the arrays by)
            _l.check(self._L.fb_fem_detach_part(self.h, int(k), flags, C.byref(out), None, None, None))
        t = self.part_table()
        ids, nodes = np.zeros(int(t["elements"][k]), np.int32), np.zeros(int(t["nodes"][k]), np.int32)
        info = _l.DetachInfo()
        _l.check(self._L.fb_fem_detach_part(self.h, int(k), flags, C.byref(out), _l.iptr(ids), _l.iptr(nodes), C.byref(info)))
        piece = FemIntegrator.__new__(FemIntegrator)
        piece._L, piece.h = self._L, out
        piece.verts, piece.tets = piece.read_mesh() if track else (None, None)
        piece.n_nodes, piece.n_tets_global = int(info.n_nodes), int(info.n_elements)
        piece.r = 3 * piece.n_nodes
        piece.node_lo, piece.node_hi = 0, piece.n_nodes
        piece.params = _l.FemParams.from_buffer_copy(self.params)
        piece.last = _l.StepInfo()
        piece._embed_n = {}
        piece.detach_info = {name: getattr(info, name) for name, _ in _l.DetachInfo._fields_}
        if remove:
            self.tets = self.read_mesh()[1] if track and self.tets is not None else None
            self.n_tets_global = int(info.parent_elements_left)
        return piece, ids, nodes

    def constrained_dofs(self):
        """The constrained DOFs of the handle in the caller's ids, ascending (fb_fem_read_constrained_dofs): the list a later
        ``resync_delta`` of this handle is to be given"""
        n = int(self._L.fb_fem_num_constrained_dofs(self.h))
        out = np.zeros(max(n, 0), np.int32)
        _l.check(self._L.fb_fem_read_constrained_dofs(self.h, _l.iptr(out)))
        return out

    def time_parts(self, reps=20):
        """(seconds per labelling, seconds per split): medians of ``reps`` HIP-event timings each (fb_fem_time_parts)"""
        a, b = C.c_double(0), C.c_double(0)
        _l.check(self._L.fb_fem_time_parts(self.h, reps, C.byref(a), C.byref(b)))
        return a.value, b.value

    def resync_path(self):
        """FB_RESYNC_* of the handle's last (re-)build"""
        return int(self._L.fb_fem_resync_path(self.h))

    def rebuild_elements(self):
        _l.check(self._L.fb_fem_rebuild_elements(self.h))

    # -- IntegratorBase surface --
    def set_external_forces(self, f):
        _l.check(self._L.fb_fem_set_external_forces(self.h, _l.dptr(_l.as_f64(f, self.r))))

    def add_external_forces(self, f):
        _l.check(self._L.fb_fem_add_external_forces(self.h, _l.dptr(_l.as_f64(f, self.r))))

    def set_external_forces_to_zero(self):
        _l.check(self._L.fb_fem_set_external_forces_zero(self.h))

    def set_uniform_force(self, axis, value):
        _l.check(self._L.fb_fem_set_uniform_force(self.h, axis, value))

    def external_forces(self):
        """The external force vector the next step will read, (3 n_nodes,) in the caller's node order (fb_fem_get_external_forces)"""
        f = np.zeros(3 * int(self._L.fb_fem_num_nodes(self.h)))
        _l.check(self._L.fb_fem_get_external_forces(self.h, _l.dptr(f)))
        return f

    def do_timestep(self):
        """Returns the PCG iteration count; raises FbError(FB_ESOLVER) when the solve fails."""
        _l.check(self._L.fb_fem_step(self.h, C.byref(self.last)))
        return self.last.cg_iterations

    def get_q_state(self):
        q, qv, qa = np.zeros(self.r), np.zeros(self.r), np.zeros(self.r)
        _l.check(self._L.fb_fem_get_state(self.h, _l.dptr(q), _l.dptr(qv), _l.dptr(qa)))
        return q, qv, qa

    def set_q_state(self, q, qvel=None, qaccel=None):
        qv = None if qvel is None else _l.as_f64(qvel, self.r)
        qa = None if qaccel is None else _l.as_f64(qaccel, self.r)
        _l.check(self._L.fb_fem_set_state(self.h, _l.dptr(_l.as_f64(q, self.r)), _l.dptr(qv), _l.dptr(qa)))

    def set_newmark(self, beta=0.25, gamma=0.5, max_newton_iterations=1, epsilon=1e-6):
        _l.check(self._L.fb_fem_set_newmark(self.h, beta, gamma, max_newton_iterations, epsilon))

    def reset_to_rest(self):
        _l.check(self._L.fb_fem_reset(self.h))

    def set_timestep(self, h):
        _l.check(self._L.fb_fem_set_timestep(self.h, h))

    def set_damping(self, mass_coef, stiffness_coef):
        _l.check(self._L.fb_fem_set_damping(self.h, mass_coef, stiffness_coef))

    def set_internal_force_scaling_factor(self, factor):
        _l.check(self._L.fb_fem_set_internal_force_scaling(self.h, factor))

    # -- per-element materials (fb_fem_set_materials / fb_fem_set_element_materials; unsharded handles) --
    def set_materials(self, E, nu, rho, element_ids=None):
        """The material table: E, nu, rho scalars or equally long sequences of 1 .. ``lib.FB_MAX_MATERIALS`` entries; entry 0 is the
        material of every element without an id.  ``element_ids`` (one id per element, caller's element order) sets the whole map
        in the same call.  The reference reads each element's material (corotationalLinearFEM.cpp:55-66, tetMesh.cpp:171)."""
        E, nu, rho = (np.atleast_1d(np.asarray(a, np.float64)).reshape(-1) for a in (E, nu, rho))
        if not (len(E) == len(nu) == len(rho)):
            raise ValueError("E, nu and rho must be equally long")
        E, nu, rho = (np.ascontiguousarray(a) for a in (E, nu, rho))
        _l.check(self._L.fb_fem_set_materials(self.h, len(E), _l.dptr(E), _l.dptr(nu), _l.dptr(rho)))
        if element_ids is not None:
            self.set_element_materials(element_ids)

    def set_element_materials(self, ids, first=0):
        """Material ids (0 .. 255, below the table's length) of elements first .. first + len(ids) - 1 in the caller's element order"""
        a = np.asarray(ids).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 255):
            raise ValueError("material ids are 0 .. 255")
        a = np.ascontiguousarray(a, dtype=np.uint8)
        _l.check(self._L.fb_fem_set_element_materials(self.h, int(first), len(a), _l.bptr(a)))

    def materials(self):
        """(E, nu, rho) arrays of the table, as set (the internal force scaling factor is not folded in)"""
        n = int(self._L.fb_fem_num_materials(self.h))
        E, nu, rho = np.zeros(n), np.zeros(n), np.zeros(n)
        _l.check(self._L.fb_fem_read_materials(self.h, _l.dptr(E), _l.dptr(nu), _l.dptr(rho)))
        return E, nu, rho

    def element_materials(self):
        """The material id of every element of the mesh the device holds (uint8, ``read_mesh``'s element order)"""
        ids = np.zeros(int(self._L.fb_fem_num_tets(self.h)), np.uint8)
        _l.check(self._L.fb_fem_read_element_materials(self.h, 0, len(ids), _l.bptr(ids)))
        return ids

    def element_map_bytes(self):
        """Bytes the element map holds on the device; 0 for a handle that never got a non-zero id (it allocates none)"""
        return int(self._L.fb_fem_element_map_bytes(self.h))

    def set_cg(self, eps, max_iter):
        _l.check(self._L.fb_fem_set_cg(self.h, eps, max_iter))

    def set_constrained_dofs(self, fixed_dofs):
        fd = _l.as_i32(fixed_dofs)
        _l.check(self._L.fb_fem_set_constrained_dofs(self.h, len(fd), _l.iptr(fd)))

    def get_force_assembly_time(self):
        return self.last.assembly_seconds

    def get_system_solve_time(self):
        return self.last.solve_seconds

    def floor_collision(self, floor_y, restitution=0.4):
        n = C.c_int(0)
        _l.check(self._L.fb_fem_floor_collision(self.h, floor_y, restitution, C.byref(n)))
        return n.value

    # -- the haptic probe on the device (fb_fem_add_haptic_forces / pick / volume; unsharded handles) --
    def add_haptic_forces(self, indices, forces, neighborhood_size):
        """``Deformable::applyHapticForces`` on the device: adds ``forces[s]`` to node ``indices[s]`` and, with the fall-off
        (size - j) / size, to the nodes of ring j = 1 .. size-1 around it -- into the current external force vector, bit for bit what
        ``spread_haptic_forces`` adds.  At most ``lib.FB_HAPTIC_MAX_SOURCES`` sources."""
        ids = _l.as_i32(indices)
        f = _l.as_f64(forces, 3 * len(ids))
        _l.check(self._L.fb_fem_add_haptic_forces(self.h, len(ids), _l.iptr(ids), _l.dptr(f), int(neighborhood_size)))

    def pick_vertex(self, wpos):
        """(index, position (3,), squared distance) of the node closest to ``wpos`` at the current state; of equal distances the lowest id"""
        w = _l.as_f64(wpos, 3)
        idx, xyz, d2 = C.c_int(-1), np.zeros(3), C.c_double(0)
        _l.check(self._L.fb_fem_pick_vertex(self.h, _l.dptr(w), C.byref(idx), _l.dptr(xyz), C.byref(d2)))
        return idx.value, xyz, d2.value

    def pick_box(self, lo, hi, capacity=None, ids=None, xyz=None):
        """(count, ids, positions) of the nodes with lo <= x0 + q <= hi, ascending ids.  capacity None: room for every node; 0: the
        count only (ids and positions None).  ids / xyz: the caller's arrays to fill (at least ``capacity`` / ``3 capacity`` long);
        only the first min(count, capacity) entries are written, and the returned views end there."""
        lo, hi = _l.as_f64(lo, 3), _l.as_f64(hi, 3)
        cap = self.n_nodes if capacity is None else int(capacity)
        n = C.c_int(0)
        if cap == 0:
            _l.check(self._L.fb_fem_pick_box(self.h, _l.dptr(lo), _l.dptr(hi), 0, None, None, C.byref(n)))
            return n.value, None, None
        ids = np.zeros(cap, np.int32) if ids is None else ids
        xyz = np.zeros((cap, 3)) if xyz is None else xyz
        if ids.dtype != np.int32 or xyz.dtype != np.float64 or ids.size < cap or xyz.size < 3 * cap or not (ids.flags.c_contiguous and xyz.flags.c_contiguous):
            raise ValueError("ids: contiguous int32 of at least capacity, xyz: contiguous float64 of at least 3 capacity")
        _l.check(self._L.fb_fem_pick_box(self.h, _l.dptr(lo), _l.dptr(hi), cap, _l.iptr(ids), _l.dptr(xyz), C.byref(n)))
        m = min(n.value, cap)
        return n.value, ids.reshape(-1)[:m], xyz.reshape(-1)[:3 * m].reshape(m, 3)

    def volume(self, per_element=False):
        """Volume of the mesh at the current state (``Deformable::computeVolume``); with ``per_element`` (total, volumes (n_tets,)) in
        ``read_mesh``'s element order"""
        t = C.c_double(0)
        pe = np.zeros(int(self._L.fb_fem_num_tets(self.h))) if per_element else None
        _l.check(self._L.fb_fem_volume(self.h, C.byref(t), _l.dptr(pe)))
        return (t.value, pe) if per_element else t.value

    # -- the probe's box contact on the device (fb_fem_contact_move / apply; unsharded handles) --
    @staticmethod
    def _contact_info(c):
        return dict(status=c.status, n_touched=c.n_touched, n_new=c.n_new, face=c.face, closest_node=c.closest_node, n_pushing=c.n_pushing,
                    list_size=c.list_size, n_clears=c.n_clears, contact_dist=c.contact_dist, closest_point=np.array(c.closest_point[:], np.float64))

    def contact_move(self, lo, hi, force_coeff):
        """``AvatarProbe::onTranslate`` below its pick-mode branch, on the device: the tool box [lo, hi] against the tissue -- miss test,
        touched set with first-touch positions, contact face, penalty forces.  The list stays on the device (``contact_apply`` spreads
        it); the info dict comes back.  What ``ProbeContact.move`` computes on the host."""
        lo, hi = _l.as_f64(lo, 3), _l.as_f64(hi, 3)
        c = _l.ContactInfo()
        _l.check(self._L.fb_fem_contact_move(self.h, _l.dptr(lo), _l.dptr(hi), float(force_coeff), C.byref(c)))
        return self._contact_info(c)

    def contact_info(self):
        """The contact session's state without a move"""
        c = _l.ContactInfo()
        _l.check(self._L.fb_fem_contact_info_get(self.h, C.byref(c)))
        return self._contact_info(c)

    def contact_reset(self, keep_face=True):
        """Clears the touched set and the force list; ``keep_face`` keeps the contact face (the reference's mouse-up), False is a new probe"""
        _l.check(self._L.fb_fem_contact_reset(self.h, 1 if keep_face else 0))

    def read_contact(self):
        """(ids (k,), first-touch positions (k, 3), forces (k, 3)) of the stored list, ascending ids"""
        k = self.contact_info()["list_size"]
        ids, first, f = np.zeros(k, np.int32), np.zeros((k, 3)), np.zeros((k, 3))
        if k:
            _l.check(self._L.fb_fem_read_contact(self.h, _l.iptr(ids), _l.dptr(first), _l.dptr(f)))
        return ids, first, f

    def contact_apply(self, neighborhood_size):
        """``Deformable::applyHapticForces`` on the stored contact list, added into the current external force vector; any number of
        sources.  Returns dict(n_sources, n_pushing, path, n_targets, n_records)."""
        c = _l.ContactSpreadInfo()
        _l.check(self._L.fb_fem_contact_apply(self.h, int(neighborhood_size), C.byref(c)))
        return dict(n_sources=c.n_sources, n_pushing=c.n_pushing, path=c.path, n_targets=c.n_targets, n_records=c.n_records)

    # -- contact between two bodies on the device (fb_fem_body_contact; unsharded handles on one device) --
    _BODY_DIRECTIONS = {"both": _l.FB_BODY_A_INTO_B | _l.FB_BODY_B_INTO_A, "a_into_b": _l.FB_BODY_A_INTO_B, "b_into_a": _l.FB_BODY_B_INTO_A}

    def _body_params(self, stiffness, depth_cap, directions):
        p = _l.BodyContactParams()
        p.stiffness, p.depth_cap = float(stiffness), float(depth_cap)
        p.directions = self._BODY_DIRECTIONS[directions] if isinstance(directions, str) else int(directions)
        return p

    @staticmethod
    def _friction_params(mu, slip_speed, damping):
        fr = _l.ContactFrictionParams()
        fr.mu, fr.slip_speed, fr.damping, fr.reserved = float(mu), float(slip_speed), float(damping), 0.0
        return fr

    @staticmethod
    def _friction_info(fi):
        return dict(n_sticking=tuple(fi.n_sticking), n_sliding=tuple(fi.n_sliding), n_separating=tuple(fi.n_separating), max_slip_speed=float(fi.max_slip_speed),
                    max_normal_force=float(fi.max_normal_force), max_stick_rate=float(fi.max_stick_rate),
                    friction_on_points=np.array([fi.friction_on_points[0][:], fi.friction_on_points[1][:]]))

    def body_contact(self, other, stiffness, depth_cap=0.0, directions="both", mu=0.0, slip_speed=0.0, damping=0.0):
        """Penalty contact between this body (a) and ``other`` (b) at their current states, ADDED into both external force vectors (set
        gravity or zero first): every surface vertex of one body that lies inside an element of the other is pushed to the closest point
        of the other's boundary with F = stiffness * min(depth, depth_cap) * n (no cap where depth_cap is 0), and the face that holds that
        point is pushed back by -F, spread by its weights.  directions: "both", "a_into_b" (this body's vertices in ``other``), "b_into_a",
        or the FB_BODY_* bits.  Returns the dict of the fb_fem_body_contact_info fields; counts are (a into b, b into a).
        mu, slip_speed, damping: with any of them non-zero the force law is fb_fem_body_contact_friction's -- regularised Coulomb friction
        (linear below slip_speed, mu N at and above it) and a damper along the normal, from the two bodies' velocities; explicit, so keep
        mu N / slip_speed * dt and damping * dt below the mass a contact pushes (``max_stick_rate`` comes back for that).  The dict then
        also holds the fb_fem_contact_friction_info fields."""
        p, info = self._body_params(stiffness, depth_cap, directions), _l.BodyContactInfo()
        friction = None
        if mu == 0.0 and slip_speed == 0.0 and damping == 0.0:
            _l.check(self._L.fb_fem_body_contact(self.h, other.h, C.byref(p), C.byref(info)))
        else:
            fr, fi = self._friction_params(mu, slip_speed, damping), _l.ContactFrictionInfo()
            _l.check(self._L.fb_fem_body_contact_friction(self.h, other.h, C.byref(p), C.byref(fr), C.byref(info), C.byref(fi)))
            friction = self._friction_info(fi)
        out = dict(n_candidates=tuple(info.n_candidates), n_contacts=tuple(info.n_contacts), n_degenerate=tuple(info.n_degenerate), path=int(info.path),
                   n_tet_grid_builds=int(info.n_tet_grid_builds), n_face_grid_builds=int(info.n_face_grid_builds), faces_tested=int(info.faces_tested),
                   max_depth=float(info.max_depth), force_on_a=np.array(info.force_on_a[:]), force_on_b=np.array(info.force_on_b[:]))
        self._body_contacts = out["n_contacts"]
        if friction is not None:
            out.update(friction)
            self._body_friction_contacts = out["n_contacts"]
        return out

    def read_body_contact_friction(self, direction):
        """Per contact of one direction of the last ``body_contact`` that ran with friction or damping, in ``read_body_contact``'s order:
        dict of normal_force (k,) N, slip (k, 3) the tangential velocity of the point relative to the face, and friction (k, 3) the
        friction on the point's node, -f."""
        d = self._BODY_DIRECTIONS[direction] if isinstance(direction, str) else int(direction)
        if d not in (_l.FB_BODY_A_INTO_B, _l.FB_BODY_B_INTO_A):
            raise ValueError("one direction, not %r" % (direction,))
        k = getattr(self, "_body_friction_contacts", (0, 0))[0 if d == _l.FB_BODY_A_INTO_B else 1]
        N, slip, friction = np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3))
        _l.check(self._L.fb_fem_read_body_contact_friction(self.h, d, _l.dptr(N), _l.dptr(slip), _l.dptr(friction)))
        return dict(normal_force=N, slip=slip, friction=friction)

    def read_body_contact(self, direction):
        """The contacts of one direction ("a_into_b" / "b_into_a" or the FB_BODY_* bit) of the last ``body_contact`` of this handle: dict of
        node (the vertex, in its body's ids), element and face (of the other body: ``read_mesh`` / ``surface`` order), closest (k, 3), bary
        (k, 3) the weights of the closest point on the face's corners, and depth (k,) before the cap; ascending node."""
        d = self._BODY_DIRECTIONS[direction] if isinstance(direction, str) else int(direction)
        if d not in (_l.FB_BODY_A_INTO_B, _l.FB_BODY_B_INTO_A):
            raise ValueError("one direction, not %r" % (direction,))
        k = getattr(self, "_body_contacts", (0, 0))[0 if d == _l.FB_BODY_A_INTO_B else 1]
        node, elem, face = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        closest, bary, depth = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k)
        _l.check(self._L.fb_fem_read_body_contact(self.h, d, _l.iptr(node), _l.iptr(elem), _l.iptr(face), _l.dptr(closest), _l.dptr(bary), _l.dptr(depth)))
        return dict(node=node, element=elem, face=face, closest=closest, bary=bary, depth=depth)

    def time_body_contact(self, other, stiffness, depth_cap=0.0, directions="both", reps=5):
        """Seconds of the five stages of ``body_contact`` (boxes, element grid and containment, face grid, closest faces, scatter), means of
        ``reps`` runs with their host waits (fb_fem_time_body_contact).  Adds no force."""
        p, sec = self._body_params(stiffness, depth_cap, directions), np.zeros(5)
        _l.check(self._L.fb_fem_time_body_contact(self.h, other.h, C.byref(p), int(reps), _l.dptr(sec)))
        return sec

    # -- contact of the body with itself on the device (fb_fem_self_contact; unsharded handles) --
    _SELF_MODES = {"any": _l.FB_SELF_CONTACT_ANY, "other_parts": _l.FB_SELF_CONTACT_OTHER_PARTS}

    def _self_params(self, stiffness, depth_cap, mode):
        p = _l.SelfContactParams()
        p.stiffness, p.depth_cap = float(stiffness), float(depth_cap)
        p.mode = self._SELF_MODES[mode] if isinstance(mode, str) else int(mode)
        return p

    def self_contact(self, stiffness, depth_cap=0.0, mode="any", mu=0.0, slip_speed=0.0, damping=0.0):
        """Penalty contact of this body with itself at its current state, ADDED into the external force vector (set gravity or zero first):
        every surface vertex that lies inside an element it may meet is pushed to the closest point of the boundary it may meet with
        F = stiffness * min(depth, depth_cap) * n (no cap where depth_cap is 0), and the face there is pushed back by -F, spread by its
        weights.  mode "any": a vertex may not meet the elements and faces that use its own node (a fold of one part); "other_parts": it may
        not meet its own part (the halves of a cut; the labels of ``parts`` are built first where they are stale); or the FB_SELF_CONTACT_*
        values.  Returns the dict of the fb_fem_self_contact_info fields.  mu, slip_speed, damping: as in ``body_contact``, through
        fb_fem_self_contact_friction; the dict then also holds the fb_fem_contact_friction_info fields (index 0 of the pairs)."""
        p, info = self._self_params(stiffness, depth_cap, mode), _l.SelfContactInfo()
        friction = None
        if mu == 0.0 and slip_speed == 0.0 and damping == 0.0:
            _l.check(self._L.fb_fem_self_contact(self.h, C.byref(p), C.byref(info)))
        else:
            fr, fi = self._friction_params(mu, slip_speed, damping), _l.ContactFrictionInfo()
            _l.check(self._L.fb_fem_self_contact_friction(self.h, C.byref(p), C.byref(fr), C.byref(info), C.byref(fi)))
            friction = self._friction_info(fi)
        out = {name: int(getattr(info, name)) for name in ("n_points", "n_contacts", "n_degenerate", "path", "n_point_grid_builds", "n_face_grid_builds",
                                                            "n_parts_builds", "faces_tested")}
        out.update(max_depth=float(info.max_depth), force_on_points=np.array(info.force_on_points[:]), force_on_faces=np.array(info.force_on_faces[:]))
        self._self_contacts = out["n_contacts"]
        if friction is not None:
            out.update(friction)
            self._self_friction_contacts = out["n_contacts"]
        return out

    def read_self_contact_friction(self):
        """Per contact of the last ``self_contact`` that ran with friction or damping, in ``read_self_contact``'s order: dict of
        normal_force (k,), slip (k, 3) and friction (k, 3) = -f."""
        k = getattr(self, "_self_friction_contacts", 0)
        N, slip, friction = np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3))
        _l.check(self._L.fb_fem_read_self_contact_friction(self.h, _l.dptr(N), _l.dptr(slip), _l.dptr(friction)))
        return dict(normal_force=N, slip=slip, friction=friction)

    def read_self_contact(self):
        """The contacts of the last ``self_contact``: dict of node (the vertex), element and face (``read_mesh`` / ``surface`` order), closest
        (k, 3), bary (k, 3) the weights of the closest point on the face's corners, and depth (k,) before the cap; ascending node."""
        k = getattr(self, "_self_contacts", 0)
        node, elem, face = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        closest, bary, depth = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k)
        _l.check(self._L.fb_fem_read_self_contact(self.h, _l.iptr(node), _l.iptr(elem), _l.iptr(face), _l.dptr(closest), _l.dptr(bary), _l.dptr(depth)))
        return dict(node=node, element=elem, face=face, closest=closest, bary=bary, depth=depth)

    def time_self_contact(self, stiffness, depth_cap=0.0, mode="any", reps=5):
        """Seconds of the five stages of ``self_contact`` (positions and box, point grid and containment, face grid, closest faces,
        scatter), means of ``reps`` runs with their host waits (fb_fem_time_self_contact).  Adds no force."""
        p, sec = self._self_params(stiffness, depth_cap, mode), np.zeros(5)
        _l.check(self._L.fb_fem_time_self_contact(self.h, C.byref(p), int(reps), _l.dptr(sec)))
        return sec

    # -- contact with a rigid tool on the device (fb_fem_tool_contact; unsharded handles) --
    _TOOL_POINTS = {"surface": _l.FB_TOOL_SURFACE_VERTICES, "all_nodes": _l.FB_TOOL_ALL_NODES}

    @staticmethod
    def _tool(shapes, origin, velocity, omega):
        """fb_tool from erosion.py's shape tuples, checked by ``erosion.check_shapes``"""
        from . import erosion
        shapes = list(shapes)
        erosion.check_shapes(shapes)
        if not 1 <= len(shapes) <= _l.FB_TOOL_MAX_SHAPES:
            raise ValueError("a tool has 1 .. %d shapes, not %d" % (_l.FB_TOOL_MAX_SHAPES, len(shapes)))
        T = _l.Tool()
        T.n_shapes = len(shapes)
        for S, s in zip(T.shapes, shapes):
            S.a[:] = _l.as_f64(s[1], 3)
            if s[0] == "sphere":
                S.kind, S.size[0] = _l.FB_TOOL_SPHERE, float(s[2])
            elif s[0] == "capsule":
                S.kind, S.size[0] = _l.FB_TOOL_CAPSULE, float(s[3])
                S.b[:] = _l.as_f64(s[2], 3)
            else:
                S.kind = _l.FB_TOOL_BOX
                S.size[:] = _l.as_f64(s[2], 3)
                S.R[:] = _l.as_f64(np.eye(3) if len(s) < 4 or s[3] is None else s[3], 9)
        T.origin[:], T.velocity[:], T.omega[:] = _l.as_f64(origin, 3), _l.as_f64(velocity, 3), _l.as_f64(omega, 3)
        return T

    def _tool_params(self, stiffness, depth_cap, points):
        p = _l.ToolContactParams()
        p.stiffness, p.depth_cap = float(stiffness), float(depth_cap)
        p.points = self._TOOL_POINTS[points] if isinstance(points, str) else int(points)
        return p

    def tool_contact(self, shapes, stiffness, depth_cap=0.0, points="surface", origin=(0, 0, 0), velocity=(0, 0, 0), omega=(0, 0, 0), mu=0.0, slip_speed=0.0,
                     damping=0.0):
        """Penalty contact of a rigid tool with this body at its current state, ADDED into the external force vector (set gravity or zero
        first).  shapes: erosion.py's tuples -- ("sphere", centre, radius), ("capsule", a, b, radius), ("box", centre, half, R) -- in the
        world frame, 1 .. 16 of them; every point (points "surface": the surface vertices; "all_nodes": every node) that a shape holds is
        pushed out along that shape's normal with F = stiffness * min(depth, depth_cap) * n (no cap where depth_cap is 0), of several
        shapes the deepest.  origin, velocity, omega: the tool's reference point, its velocity and its angular velocity;
        mu, slip_speed, damping: with any of them non-zero the force law is the friction calls' (``body_contact``), with the tool's
        velocity at the point in place of a face's.  Returns the dict of the fb_fem_tool_contact_info fields: force_on_tool and
        torque_on_tool (about origin) are what the tissue returns to the tool."""
        T, p, info = self._tool(shapes, origin, velocity, omega), self._tool_params(stiffness, depth_cap, points), _l.ToolContactInfo()
        fr = None if mu == 0.0 and slip_speed == 0.0 and damping == 0.0 else C.byref(self._friction_params(mu, slip_speed, damping))
        _l.check(self._L.fb_fem_tool_contact(self.h, C.byref(T), C.byref(p), fr, C.byref(info)))
        out = {name: int(getattr(info, name)) for name in ("n_points", "n_contacts", "n_degenerate", "n_sticking", "n_sliding", "n_separating")}
        out.update({name: float(getattr(info, name)) for name in ("max_depth", "max_slip_speed", "max_normal_force", "max_stick_rate")})
        out.update(contacts_by_shape=np.array(info.contacts_by_shape[:T.n_shapes]), force_on_body=np.array(info.force_on_body[:]),
                   force_on_tool=np.array(info.force_on_tool[:]), torque_on_tool=np.array(info.torque_on_tool[:]))
        return out

    def read_tool_contact(self):
        """The contacts of the last ``tool_contact``, ascending point: dict of node, shape (the winning one), depth (k,) before the cap,
        normal (k, 3), force (k, 3) the force added to the node, and normal_force (k,), slip (k, 3), friction (k, 3) = -f of the friction
        law (zero after a frictionless call)."""
        k = int(self._L.fb_fem_num_tool_contacts(self.h))
        if k < 0:
            _l.check(k)
        node, shape, depth, normal, force = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3))
        N, slip, friction = np.zeros(k), np.zeros((k, 3)), np.zeros((k, 3))
        _l.check(self._L.fb_fem_read_tool_contact(self.h, _l.iptr(node), _l.iptr(shape), _l.dptr(depth), _l.dptr(normal), _l.dptr(force), _l.dptr(N), _l.dptr(slip),
                                                  _l.dptr(friction)))
        return dict(node=node, shape=shape, depth=depth, normal=normal, force=force, normal_force=N, slip=slip, friction=friction)

    def time_tool_contact(self, shapes, stiffness, depth_cap=0.0, points="surface", origin=(0, 0, 0), velocity=(0, 0, 0), omega=(0, 0, 0), mu=0.0, slip_speed=0.0,
                          damping=0.0, reps=5):
        """Seconds of the three stages of ``tool_contact`` (points against shapes, compaction and the host wait, forces and the records'
        way back), means of ``reps`` runs (fb_fem_time_tool_contact).  Adds no force and leaves the records of the last call alone."""
        T, p, sec = self._tool(shapes, origin, velocity, omega), self._tool_params(stiffness, depth_cap, points), np.zeros(3)
        fr = None if mu == 0.0 and slip_speed == 0.0 and damping == 0.0 else C.byref(self._friction_params(mu, slip_speed, damping))
        _l.check(self._L.fb_fem_time_tool_contact(self.h, C.byref(T), C.byref(p), fr, int(reps), _l.dptr(sec)))
        return sec

    # -- constrained DOFs that follow a tool, and the force they return (fb_fem_set_constrained_motion / fb_fem_grasp; unsharded handles) --
    def set_constrained_motion(self, dofs, displacements):
        """Replaces the motion set: ``dofs`` (caller ids, ascending, each a constrained DOF of the handle) end the next ``do_timestep``
        at ``displacements`` bit for bit, with qvel = (u - q) / h; the free DOFs feel them through the matrix columns the stored matrix
        does not hold, as a right-hand-side correction.  The targets stay until they are changed; an empty list clears the set.  A target
        far from q is a large velocity in one step: move it a little per step."""
        d = np.ascontiguousarray(dofs, np.int32).reshape(-1)
        u = np.ascontiguousarray(displacements, np.float64).reshape(-1)
        if len(d) != len(u):
            raise ValueError("one displacement per DOF")
        _l.check(self._L.fb_fem_set_constrained_motion(self.h, len(d), _l.iptr(d), _l.dptr(u)))

    def constrained_motion(self):
        """(dofs, displacements) of the motion set (fb_fem_read_constrained_motion)"""
        n = max(int(self._L.fb_fem_num_constrained_motion(self.h)), 0)
        d, u = np.zeros(n, np.int32), np.zeros(n)
        _l.check(self._L.fb_fem_read_constrained_motion(self.h, _l.iptr(d), _l.dptr(u)))
        return d, u

    def reactions(self):
        """(forces, sum3): the force the constraint put on the body at every DOF of the motion set during the last step, in the set's
        order, and its sum by axis (fb_fem_read_reactions); zeros before a step with the set.  A haptic device is fed ``-sum3``."""
        n = max(int(self._L.fb_fem_num_constrained_motion(self.h)), 0)
        f, s = np.zeros(n), np.zeros(3)
        _l.check(self._L.fb_fem_read_reactions(self.h, _l.dptr(f), _l.dptr(s)))
        return f, s

    def motion_info(self):
        """dict of the fb_fem_motion_info fields: n_dofs, n_listed_elements, n_touched_nodes, longest_run, table_builds, table_valid, n_grasp_nodes"""
        info = _l.MotionInfo()
        _l.check(self._L.fb_fem_motion_info_get(self.h, C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in _l.MotionInfo._fields_ if name != "reserved"}

    def time_motion(self, reps=5):
        """Seconds of the table build, the right-hand-side correction, the reactions and the write of the moved DOFs, means of ``reps``
        runs (fb_fem_time_motion); state and reactions stay what they are."""
        sec = np.zeros(4)
        _l.check(self._L.fb_fem_time_motion(self.h, int(reps), _l.dptr(sec)))
        return sec

    def grasp(self, nodes):
        """Holds ``nodes`` (caller ids, ascending): their DOFs join the constrained list and the motion set with their current q as the
        target, their world positions are remembered (fb_fem_grasp).  Returns ``motion_info()``."""
        ids = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        info = _l.MotionInfo()
        _l.check(self._L.fb_fem_grasp(self.h, len(ids), _l.iptr(ids), C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in _l.MotionInfo._fields_ if name != "reserved"}

    def grasp_move(self, R=None, t=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
        """Targets of the grasped nodes = R (p_grab - pivot) + pivot + t - x0, set on the device (fb_fem_grasp_move); R 3x3, row-major"""
        R = np.eye(3) if R is None else R
        _l.check(self._L.fb_fem_grasp_move(self.h, _l.dptr(_l.as_f64(R, 9)), _l.dptr(_l.as_f64(t, 3)), _l.dptr(_l.as_f64(pivot, 3))))

    def release(self):
        """Lets go: what ``grasp`` added leaves the constrained list and the motion set, q and qvel stay (fb_fem_release)"""
        _l.check(self._L.fb_fem_release(self.h))

    # -- element stress and strain on the device (fb_fem_stress / read_stress / surface_stress; unsharded handles) --
    def stress(self, world=False, tensors=False):
        """Stress and strain of every element at the current state, kept on the device (fb_fem_stress): the bracket of the corotational
        element force, sigma = lambda tr(H) I + mu (H + H^T) with the assembly's rotation.  Returns the summary: dict of n_elements, flags,
        max_von_mises / max_element, min_J / min_J_element (of equal values the lowest element), n_inverted (J < 0) and energy
        (sum of V psi).  ``tensors`` keeps the six-vectors (xx yy zz xy yz zx, tensor components) for ``element_stress``; ``world``
        stores them rotated to the world frame instead of the element's rest frame."""
        info = _l.StressInfo()
        flags = (_l.FB_STRESS_WORLD if world else 0) | (_l.FB_STRESS_TENSORS if tensors else 0)
        _l.check(self._L.fb_fem_stress(self.h, flags, C.byref(info)))
        return {name: getattr(info, name) for name, _ in _l.StressInfo._fields_}

    def element_stress(self, first=0, count=None, tensors=None):
        """The arrays of the last ``stress()`` for elements first .. first + count - 1 (``read_mesh``'s element order): dict of
        von_mises, energy_density, J (count,) and, where that call kept tensors, stress and strain (count, 6).  ``tensors=True`` asks
        for the six-vectors and raises where they were not kept; False leaves them out.  Raises FbError(FB_EINVAL) when there is no
        ``stress()`` of the current mesh."""
        if count is None:
            count = int(self._L.fb_fem_num_tets(self.h)) - int(first)
        n = max(int(count), 0)
        out = dict(von_mises=np.zeros(n), energy_density=np.zeros(n), J=np.zeros(n))
        if tensors is None:  # whatever the last call kept: the library says (an empty range with a tensor pointer is refused where none were kept)
            _l.check(self._L.fb_fem_read_stress(self.h, 0, 0, None, None, None, None, None))   # (no stress of this mesh: raise that)
            probe = np.zeros(6)
            tensors = self._L.fb_fem_read_stress(self.h, 0, 0, None, None, None, _l.dptr(probe), None) == _l.FB_OK
        if tensors:
            out["stress"], out["strain"] = np.zeros((n, 6)), np.zeros((n, 6))
        _l.check(self._L.fb_fem_read_stress(self.h, int(first), int(count), _l.dptr(out["von_mises"]), _l.dptr(out["energy_density"]), _l.dptr(out["J"]),
                                            _l.dptr(out.get("stress")), _l.dptr(out.get("strain"))))
        return out

    def surface_stress(self):
        """(V,) float32: per surface vertex, in ``surface()['vertex_ids']`` order, the mean von Mises stress of the elements behind its
        faces, from the last ``stress()`` (fb_fem_surface_stress) -- the colour to draw on ``surface_update()``'s vertices"""
        info = _l.SurfaceInfo()
        _l.check(self._L.fb_fem_read_stress(self.h, 0, 0, None, None, None, None, None))  # (stale: raise before the surface is built)
        _l.check(self._L.fb_fem_surface(self.h, C.byref(info)))
        vm = np.zeros(info.n_vertices, np.float32)
        _l.check(self._L.fb_fem_surface_stress(self.h, _l.fptr(vm)))
        return vm

    def time_stress(self, reps=20, world=False, tensors=False):
        """(seconds per stress(), seconds per surface_stress()): medians of ``reps`` HIP-event timings each (fb_fem_time_stress)"""
        a, b = C.c_double(0), C.c_double(0)
        flags = (_l.FB_STRESS_WORLD if world else 0) | (_l.FB_STRESS_TENSORS if tensors else 0)
        _l.check(self._L.fb_fem_time_stress(self.h, reps, flags, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- inspection (parity tests) --
    def num_tets(self):
        return self._L.fb_fem_num_tets(self.h)

    def num_blocks(self):
        return self._L.fb_fem_num_blocks(self.h)

    def matrix_precision(self):
        """lib.FB_MATRIX_F32 / FB_MATRIX_F64: the width the matrix values are stored in (FB_MATRIX_AUTO decides by size)"""
        return int(self._L.fb_fem_matrix_precision(self.h))

    def pattern(self):
        n_owned = self.node_hi - self.node_lo
        bptr, bcol = np.empty(n_owned + 1, np.int32), np.empty(self.num_blocks(), np.int32)
        _l.check(self._L.fb_fem_pattern(self.h, _l.iptr(bptr), _l.iptr(bcol)))
        return bptr, bcol

    def element_stiffness(self, first, count):
        K0, Mi = np.empty((count, 12, 12)), np.empty((count, 4, 4))
        _l.check(self._L.fb_fem_element_stiffness(self.h, first, count, _l.dptr(K0), _l.dptr(Mi)))
        return K0, Mi

    def assemble(self, u):
        f, K = np.zeros(self.r), np.empty((self.num_blocks(), 3, 3))
        _l.check(self._L.fb_fem_assemble(self.h, _l.dptr(_l.as_f64(u, self.r)), _l.dptr(f), _l.dptr(K)))
        return f, K

    def system(self):
        rhs, K = np.zeros(self.r), np.empty((self.num_blocks(), 3, 3))
        _l.check(self._L.fb_fem_system(self.h, _l.dptr(K), _l.dptr(rhs)))
        return K, rhs

    def mass(self):
        m = np.empty(self.num_blocks())
        _l.check(self._L.fb_fem_mass(self.h, _l.dptr(m)))
        return m

    def spmv(self, x):
        y = np.zeros(self.r)
        _l.check(self._L.fb_fem_spmv(self.h, _l.dptr(_l.as_f64(x, self.r)), _l.dptr(y)))
        return y

    def pcg(self, rhs, eps=1e-6, max_iter=10000):
        x, it = np.zeros(self.r), C.c_int(0)
        _l.check(self._L.fb_fem_pcg(self.h, _l.dptr(_l.as_f64(rhs, self.r)), _l.dptr(x), eps, max_iter, C.byref(it)))
        return it.value, x

    def time_spmv(self, reps=50):
        s = C.c_double(0)
        _l.check(self._L.fb_fem_time_spmv(self.h, reps, C.byref(s)))
        return s.value

    def persist_info(self):
        """(runs persistent PCG launches?, wavefronts per CU, workgroups, LDS-resident slots per slice)"""
        w, b, k = C.c_int(0), C.c_int(0), C.c_int(0)
        on = self._L.fb_fem_persist_info(self.h, C.byref(w), C.byref(b), C.byref(k))
        return bool(on == 1), w.value, b.value, k.value

    def persist_gather(self):
        """(published vector node by node?, cache lines a slot's gathers touch in planes, in 24-byte records) -- fb_fem_persist_gather"""
        a, b = C.c_double(0), C.c_double(0)
        on = self._L.fb_fem_persist_gather(self.h, C.byref(a), C.byref(b))
        return bool(on), a.value, b.value

    def persist_mirror(self):
        """(some layer mirrored?, mirror layers over all slices, pool entries, fewest plain LDS slots of a slice) -- fb_fem_persist_mirror"""
        m, p, k = C.c_int(0), C.c_int(0), C.c_int(0)
        on = self._L.fb_fem_persist_mirror(self.h, C.byref(m), C.byref(p), C.byref(k))
        if on < 0:
            _l.check(on)
        return bool(on == 1), m.value, p.value, k.value

    def persist_regs(self):
        """(register slots a slice holds at most: 0, 2 or 3; register slots over all slices) -- fb_fem_persist_regs"""
        r = C.c_int(0)
        total = self._L.fb_fem_persist_regs(self.h, C.byref(r))
        if total < 0:
            _l.check(total)
        return r.value, total

    def persist_prio(self):
        """The wavefront-priority form of this handle's persistent launches (FEMBRAIN_PIPE_PRIO: 1 progress, 2 static, 3 progress + service
        wavefront), 0 where the kernel has none -- fb_fem_persist_prio"""
        return int(self._L.fb_fem_persist_prio(self.h))

    def pcg_path(self):
        """What ran: dict(path = FB_PCG_PATH_* of the last solve, kernel = the persistent instantiation this handle launches or '',
        launches, fallbacks, max_producers)"""
        name = C.create_string_buffer(96)
        nl, nf, mp = C.c_int(0), C.c_int(0), C.c_int(0)
        path = self._L.fb_fem_pcg_path(self.h, name, 96, C.byref(nl), C.byref(nf), C.byref(mp))
        return dict(path=path, kernel=name.value.decode(), launches=nl.value, fallbacks=nf.value, max_producers=mp.value)

    def persist_stats(self):
        """(persistent launches of this handle's solves so far, their device seconds, the PCG iterations they ran)"""
        n, sec, it = C.c_int(0), C.c_double(0), C.c_longlong(0)
        _l.check(self._L.fb_fem_persist_stats(self.h, C.byref(n), C.byref(sec), C.byref(it)))
        return n.value, sec.value, it.value

    def time_persist(self, reps=10, n_iters=29):
        s = C.c_double(0)
        _l.check(self._L.fb_fem_time_persist(self.h, reps, n_iters, C.byref(s)))
        return s.value

    def iteration_bytes(self):
        b = C.c_double(0)
        _l.check(self._L.fb_fem_iteration_bytes(self.h, C.byref(b)))
        return b.value

    def time_assembly(self, reps=10):
        s = C.c_double(0)
        _l.check(self._L.fb_fem_time_assembly(self.h, reps, C.byref(s)))
        return s.value

    def spmv_bytes(self):
        b = C.c_double(0)
        _l.check(self._L.fb_fem_spmv_bytes(self.h, C.byref(b)))
        return b.value

    def assembly_bytes(self):
        b = C.c_double(0)
        _l.check(self._L.fb_fem_assembly_bytes(self.h, C.byref(b)))
        return b.value


def bsr_to_scipy(bptr, bcol, blocks, n_cols_nodes=None):
    """3x3-block CSR (fb_fem_pattern order) -> scipy CSR, for comparisons in the tests."""
    import scipy.sparse as sp
    n_rows = len(bptr) - 1
    n_cols = n_cols_nodes if n_cols_nodes is not None else n_rows
    return sp.bsr_matrix((np.asarray(blocks).reshape(-1, 3, 3), bcol, bptr), shape=(3 * n_rows, 3 * n_cols)).tocsr()


def spread_haptic_forces(bptr, bcol, indices, forces, neighborhood_size, ext_forces):
    """``Deformable::applyHapticForces`` (reference src/deformable/Deformable.cpp:634-706): the force of each haptic
    vertex is added to it and, with the linear fall-off (size - j) / size, to the vertices first reached in ring
    j = 1 .. size-1 of a breadth-first walk over mesh edges.  Node neighbours are the off-diagonal columns of the
    stiffness pattern (= vertices sharing a tet edge; the reference's ``VolMesh::get_node_neighbors`` intends exactly
    that set -- its ``const_edgeAt(i)`` indexing slip, VolMesh.cpp:1346-1363, is not reproduced).  Adds in place."""
    for idx, frc in zip(indices, forces):
        ext_forces[3 * idx:3 * idx + 3] += frc
    for idx, frc in zip(indices, forces):
        affected, last = {int(idx)}, {int(idx)}
        for j in range(1, neighborhood_size):
            mag = 1.0 * (neighborhood_size - j) / float(neighborhood_size)
            new = set()
            for vtx in last:
                for nb in bcol[bptr[vtx]:bptr[vtx + 1]]:
                    nb = int(nb)
                    if nb != vtx and nb not in affected:
                        new.add(nb)
            last = set()
            for nb in sorted(new):
                ext_forces[3 * nb:3 * nb + 3] += mag * np.asarray(frc, dtype=np.float64)
                last.add(nb)
                affected.add(nb)
    return ext_forces


class ProbeContact:
    """``AvatarProbe::onTranslate`` (reference src/deformable/AvatarProbe.cpp:124-265) below its pick-mode branch, on the host: the tool
    box against the tissue, the hash of touched nodes with their first-touch positions (a dict keyed by node id, walked in sorted
    order as the reference's std::map is), the contact face and the penalty forces.  What ``FemIntegrator.contact_move`` runs on
    the device; field by field the same info."""

    FACES = ("LEFT", "RIGHT", "BOTTOM", "TOP", "NEAR", "FAR")
    NORMALS = np.array([[-1.0, 0, 0], [1.0, 0, 0], [0, -1.0, 0], [0, 1.0, 0], [0, 0, -1.0], [0, 0, 1.0]])

    def __init__(self):
        self.n_clears = 0
        self.hash = {}
        self.reset(keep_face=False)

    def reset(self, keep_face=True):
        self.hash = {}
        self.ids, self.forces = np.zeros(0, np.int32), np.zeros((0, 3))
        self._info = dict(status=_l.FB_CONTACT_MISS, n_touched=0, n_new=0, face=self._info["face"] if keep_face else -1, closest_node=-1, n_pushing=0,
                          list_size=0, n_clears=self.n_clears, contact_dist=0.0, closest_point=np.zeros(3))

    def clear(self):
        """What a full re-sync does to the device session"""
        self.n_clears += 1
        self.reset(keep_face=False)

    def info(self):
        return dict(self._info, closest_point=self._info["closest_point"].copy())

    def read(self):
        """(ids, first-touch positions, forces) of the stored list"""
        first = np.array([self.hash[int(i)] for i in self.ids], np.float64).reshape(-1, 3)
        return self.ids.copy(), first, self.forces.copy()

    def move(self, positions, lo, hi, force_coeff):
        """positions: (n, 3) x0 + q of every node.  Returns the info dict."""
        lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all() and np.isfinite(force_coeff)):
            raise ValueError("bad tool box or force coefficient")
        p = np.asarray(positions, np.float64).reshape(-1, 3)
        # 1. AABB::intersect on the float boxes, strict
        pf = p.astype(np.float32)
        t_lo, t_hi = pf.min(axis=0), pf.max(axis=0)
        if ((t_lo >= hi.astype(np.float32)) | (t_hi <= lo.astype(np.float32))).any():
            self._info.update(status=_l.FB_CONTACT_MISS, n_new=0)
            return self.info()
        # 2. pickVertices, bounds included; a node already in the hash keeps its first position
        inside = np.nonzero(((p >= lo) & (p <= hi)).all(axis=1))[0]
        n_new = 0
        for i in inside:
            if int(i) not in self.hash:
                self.hash[int(i)] = p[i].copy()
                n_new += 1
        if not self.hash:
            self._info.update(status=_l.FB_CONTACT_EMPTY, n_new=0)
            return self.info()
        # 3. d(k, j) = (s_j - p_k) . n_j, the dot product summed left to right
        ids = np.array(sorted(self.hash), np.int32)
        first = np.array([self.hash[int(i)] for i in ids], np.float64).reshape(-1, 3)
        s = np.array([lo, hi, lo, hi, lo, hi])
        t = (s[None, :, :] - first[:, None, :]) * self.NORMALS[None, :, :]
        d = (t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]
        face = self._info["face"]
        if face < 0:
            k, face = divmod(int(np.argmin(d)), 6)  # (the first of equal minima: nodes ascending, then faces)
        else:
            k = int(np.argmin(d[:, face]))
        # 4. the forces
        v = d[:, face] * float(force_coeff)
        mag = np.where(v > 0.0, v, 0.0)
        self.ids, self.forces = ids, self.NORMALS[face][None, :] * mag[:, None]
        self._info.update(status=_l.FB_CONTACT_SET, n_touched=len(ids), n_new=n_new, face=face, closest_node=int(ids[k]), n_pushing=int((mag > 0.0).sum()),
                          list_size=len(ids), contact_dist=float(d[k, face]), closest_point=first[k].copy())
        return self.info()


class Deformable:
    """Per-step driver of ``Deformable::timestep`` (reference src/deformable/Deformable.cpp:318-420) without the
    scene-graph / GL parts: external forces (gravity -10000 per y-DOF unless a collision happened in the previous
    step, haptic forces), DoTimestep, floor collision with velocity rewrite, deformation callback."""

    GRAVITY_FORCE = -10000.0  # Deformable.cpp:335

    def __init__(self, verts, tets, fixed_vertices=(), floor_y=None, gravity=True, haptic_on_device=True, **kw):
        """haptic_on_device: haptic forces, picking and volume run on the device where the handle allows (unsharded, at most
        ``lib.FB_HAPTIC_MAX_SOURCES`` sources); False keeps the host route (what the tests compare against)."""
        self.fixed_vertices = sorted(int(v) for v in fixed_vertices)
        fd = fixed_vertices_to_dofs(self.fixed_vertices) if len(self.fixed_vertices) else np.zeros(0, np.int32)
        self.integrator = FemIntegrator(verts, tets, fd, **kw)
        self.dof = self.integrator.r
        self.gravity = bool(gravity)
        self.floor_y = floor_y
        self.ct_collided = 0
        self.ct_timestep = 0
        self.haptic_indices, self.haptic_forces = [], []
        self.haptic_in_progress = False
        self.haptic_force_neighborhood_size = 5  # DEFAULT_FORCE_NEIGHBORHOOD_SIZE, Deformable.h:41
        self._pattern = None
        self.haptic_on_device = bool(haptic_on_device) and kw.get("shard") is None
        self.probe = ProbeContact()  # the host route's contact session (probe_move)
        self._contact_list = False   # the list set last is the device session's (probe_move on the device route), not haptic_indices
        self.on_deform = None  # FOnApplyDeformations(dof, q), Deformable.h:46
        self._embed_tris = {}  # triangles of the embeddings made through embed()
        self.collision_body, self.collision_stiffness = None, 0.0  # set_collision_body
        self.collision_friction = (0.0, 0.0, 0.0)  # set_collision_body: (mu, slip_speed, damping)
        self.self_collision = None  # set_self_collision: (stiffness, depth_cap, mode, mu, slip_speed, damping)
        self.tool = None            # set_tool: (shapes, stiffness, keywords of FemIntegrator.tool_contact)
        self.last_tool_contact = None  # the info of the last collide_tool

    def collide_with(self, other, stiffness, depth_cap=0.0, mu=0.0, slip_speed=0.0, damping=0.0):
        """Penalty contact with another ``Deformable`` on the same device at the current states of both, ADDED to the external forces of
        both (``FemIntegrator.body_contact``).  ``timestep`` sets the forces anew before it steps: its callers use ``set_collision_body``.
        mu, slip_speed, damping: friction and contact damping, as in ``FemIntegrator.body_contact`` (all zero: the frictionless call)."""
        return self.integrator.body_contact(other.integrator, stiffness, depth_cap, mu=mu, slip_speed=slip_speed, damping=damping)

    def set_collision_body(self, other, stiffness=0.0, mu=0.0, slip_speed=0.0, damping=0.0):
        """Opt-in: every ``timestep`` adds the contact forces with ``other`` behind gravity and the probe, just before it steps (None: off).
        The call adds to both bodies and ``other`` sets its forces anew in its own ``timestep``, so two bodies that both step set each other."""
        self.collision_body, self.collision_stiffness = other, float(stiffness)
        self.collision_friction = (float(mu), float(slip_speed), float(damping))

    def self_collide(self, stiffness, depth_cap=0.0, mode="any", mu=0.0, slip_speed=0.0, damping=0.0):
        """Penalty contact of this body with itself at its current state, ADDED to its external forces (``FemIntegrator.self_contact``,
        with its friction and contact damping)."""
        return self.integrator.self_contact(stiffness, depth_cap, mode, mu=mu, slip_speed=slip_speed, damping=damping)

    def collide_tool(self, shapes, stiffness, **kw):
        """Penalty contact of a rigid tool -- erosion.py's shape tuples in the world frame -- with this body at its current state, ADDED
        to its external forces (``FemIntegrator.tool_contact``, with its keywords: depth_cap, points, origin, velocity, omega, mu,
        slip_speed, damping).  ``timestep`` sets the forces anew before it steps: its callers use ``set_tool``."""
        self.last_tool_contact = self.integrator.tool_contact(shapes, stiffness, **kw)
        return self.last_tool_contact

    def set_tool(self, shapes, stiffness=0.0, **kw):
        """Opt-in: every ``timestep`` applies the tool behind gravity, the probe, the collision body and the self contact, just before it
        steps (shapes None: off).  The caller sets the tool again whenever it has moved."""
        self.tool = None if shapes is None else (list(shapes), float(stiffness), dict(kw))

    def clear_tool(self):
        self.tool = None

    def tool_force(self):
        """The force the tissue returned to the tool in the last ``collide_tool`` (3,); zero before any"""
        return np.zeros(3) if self.last_tool_contact is None else self.last_tool_contact["force_on_tool"]

    def tool_torque(self):
        """... and the torque about the tool's origin (3,)"""
        return np.zeros(3) if self.last_tool_contact is None else self.last_tool_contact["torque_on_tool"]

    # -- held and moved: what IAvatar::grip() only flags (IScalpel.cpp:42-44) --
    def grip(self, nodes):
        """A tool closes on ``nodes`` (ids as ``pick_box`` returns them): they are held where they are (``FemIntegrator.grasp``)."""
        return self.integrator.grasp(np.unique(np.asarray(nodes, np.int32)))

    def move_grip(self, R=None, t=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
        """The held nodes follow the tool: rotated by R about pivot and shifted by t from where they were gripped (``grasp_move``).  The
        next ``timestep`` takes them there in one step: move a little per step."""
        self.integrator.grasp_move(R, t, pivot)

    def release_grip(self):
        """The tool opens: the held nodes are free again with the state they have (``FemIntegrator.release``)."""
        self.integrator.release()

    def grip_force(self):
        """The force the tissue returned to the tool during the last step: minus the sum of the reactions (3,)"""
        return -self.integrator.reactions()[1]

    def set_self_collision(self, stiffness=None, depth_cap=0.0, mode="other_parts", mu=0.0, slip_speed=0.0, damping=0.0):
        """Opt-in: every ``timestep`` adds the body's contact forces with itself behind gravity and the probe, just before it steps
        (stiffness None: off).  mode "other_parts" for the halves of a cut, "any" for a fold of one part."""
        self.self_collision = None if stiffness is None else (float(stiffness), float(depth_cap), mode, float(mu), float(slip_speed), float(damping))

    def set_deform_callback(self, fn):
        self.on_deform = fn

    def haptic_set_current_forces(self, indices, forces):
        self.haptic_indices, self.haptic_forces = list(indices), [tuple(f) for f in forces]
        self._contact_list = False  # (the list set last wins)

    def probe_start(self):
        """The probe's mouse-down without a picked node (AvatarProbe.cpp:108-109): haptics in progress"""
        self.haptic_start(0)

    def probe_move(self, lo, hi, force_coeff):
        """``AvatarProbe::onTranslate`` with the tool box [lo, hi]: the contact session decides the touched nodes, the face and the forces,
        and its list becomes the current haptic forces (every ``timestep`` spreads it).  On the device route nothing but the info comes
        back; on the host route ``ProbeContact`` works on the positions read back.  Returns the info dict."""
        if self.haptic_on_device:
            info = self.integrator.contact_move(lo, hi, force_coeff)
            if info["status"] == _l.FB_CONTACT_SET:
                self.haptic_indices, self.haptic_forces, self._contact_list = [], [], True
        else:
            info = self.probe.move(self._positions(), lo, hi, force_coeff)
            if info["status"] == _l.FB_CONTACT_SET:
                self.haptic_set_current_forces(self.probe.ids, self.probe.forces)
        return info

    def probe_end(self):
        """The probe's mouse-up (AvatarProbe.cpp:116-120): haptics end, the touched set is cleared, the face stays"""
        self.haptic_end()
        if self.haptic_on_device:
            self.integrator.contact_reset(keep_face=True)
        else:
            self.probe.reset(keep_face=True)

    def set_haptic_force_radius(self, radius):
        self.haptic_force_neighborhood_size = int(radius)

    def get_haptic_force_radius(self):
        return self.haptic_force_neighborhood_size

    def haptic_start(self, index):
        self.haptic_in_progress = True

    def haptic_end(self):
        self.haptic_in_progress = False
        self.haptic_indices, self.haptic_forces = [], []
        self._contact_list = False

    def timestep(self):
        it = self.integrator
        apply_gravity = self.gravity and self.ct_collided == 0
        if self.haptic_in_progress and self._contact_list:  # (the device session's list, any length)
            if apply_gravity:
                it.set_uniform_force(1, self.GRAVITY_FORCE)
            else:
                it.set_external_forces_to_zero()
            it.contact_apply(self.haptic_force_neighborhood_size)
        elif self.haptic_in_progress and self.haptic_indices and self.haptic_on_device and len(self.haptic_indices) <= _l.FB_HAPTIC_MAX_SOURCES:
            if apply_gravity:
                it.set_uniform_force(1, self.GRAVITY_FORCE)
            else:
                it.set_external_forces_to_zero()
            it.add_haptic_forces(self.haptic_indices, self.haptic_forces, self.haptic_force_neighborhood_size)
        elif self.haptic_in_progress and self.haptic_indices:
            if self.dof != it.r:  # (the mesh was cut: new nodes, new neighbours)
                self.dof, self._pattern = it.r, None
            f = np.zeros(self.dof)
            if apply_gravity:
                f[1::3] += self.GRAVITY_FORCE
            if self._pattern is None:
                self._pattern = it.pattern()
            spread_haptic_forces(self._pattern[0], self._pattern[1], self.haptic_indices, self.haptic_forces,
                                 self.haptic_force_neighborhood_size, f)
            it.set_external_forces(f)
        elif apply_gravity:
            it.set_uniform_force(1, self.GRAVITY_FORCE)
        else:
            it.set_external_forces_to_zero()
        if self.collision_body is not None:
            self.collide_with(self.collision_body, self.collision_stiffness, 0.0, *self.collision_friction)
        if self.self_collision is not None:
            self.self_collide(*self.self_collision)
        if self.tool is not None:
            self.collide_tool(self.tool[0], self.tool[1], **self.tool[2])
        iters = it.do_timestep()
        if self.floor_y is not None:
            self.ct_collided = it.floor_collision(self.floor_y, 0.4)
        self.ct_timestep += 1
        if self.on_deform is not None:
            q, _, _ = it.get_q_state()
            self.on_deform(self.dof, q)
        return iters

    def get_solver_time(self):
        return self.integrator.get_system_solve_time()

    def set_materials(self, E, nu, rho, element_ids=None):
        """``FemIntegrator.set_materials``: the body's material table and, with ``element_ids``, the material of every element"""
        self.integrator.set_materials(E, nu, rho, element_ids)

    def set_element_materials(self, ids, first=0):
        """``FemIntegrator.set_element_materials``"""
        self.integrator.set_element_materials(ids, first)

    def surface_mesh(self, update=False):
        """What the host draws: ``FemIntegrator.surface()``, or with ``update`` ``FemIntegrator.surface_update()``"""
        return self.integrator.surface_update() if update else self.integrator.surface()

    def embed(self, points, triangles=None, zero_threshold=0.0):
        """``FemIntegrator.embed``: the mesh the host draws instead of the boundary triangles, bound to the tets on the device -- what
        replaces the receiver of ``Deformable::setDeformCallback``"""
        eid = self.integrator.embed(points, triangles, zero_threshold)
        self._embed_tris[eid] = None if triangles is None else np.array(triangles, np.int32).reshape(-1, 3)  # (touch_embedded: the hit triangle's points)
        return eid

    def embedded_mesh(self, eid):
        """``FemIntegrator.embed_update``: (xyz, normals, info) of embedding ``eid`` at the current state"""
        return self.integrator.embed_update(eid)

    def embed_add_forces(self, eid, forces, point_ids=None):
        """``FemIntegrator.embed_add_forces``: forces on drawn points, added to the nodes' external forces through the binding"""
        self.integrator.embed_add_forces(eid, forces, point_ids)

    def embed_pick_ray(self, eid, origin, direction, t_max=np.inf):
        """``FemIntegrator.embed_pick_ray``: the nearest hit of a ray on the drawn triangles at the current state"""
        return self.integrator.embed_pick_ray(eid, origin, direction, t_max)

    def embed_pick_point(self, eid, wpos):
        """``FemIntegrator.embed_pick_point``: the drawn point closest to ``wpos``"""
        return self.integrator.embed_pick_point(eid, wpos)

    def embed_stress(self, eid):
        """``FemIntegrator.embed_stress``: the per-point scalar to draw on ``embedded_mesh(eid)``"""
        return self.integrator.embed_stress(eid)

    def external_forces(self):
        """``FemIntegrator.external_forces``"""
        return self.integrator.external_forces()

    def touch_embedded(self, eid, origin, direction, force, triangles=None):
        """A click on the drawn mesh: the ray's nearest hit on embedding ``eid``, and ``force`` shared among the hit triangle's three
        points by the hit's barycentrics (1-u-v, u, v), added to the external forces (``embed_add_forces`` with the three ids
        ascending).  ``triangles``: the (m, 3) array the embedding was made with (kept by ``embed`` when made through this object).
        Returns the hit (``embed_pick_ray``'s dict, with ``point_ids`` and ``forces`` as they were added); nothing is added on a miss."""
        hit = self.integrator.embed_pick_ray(eid, origin, direction)
        if hit["triangle"] < 0:
            return hit
        tri = self._embed_tris.get(eid) if triangles is None else np.asarray(triangles, np.int32).reshape(-1, 3)
        if tri is None:
            raise ValueError("embedding %r was not made with triangles through this object: pass them" % (eid,))
        u, v = hit["bary"]
        ids = tri[hit["triangle"]].astype(np.int32)
        f = np.array([1.0 - u - v, u, v])[:, None] * np.asarray(force, np.float64).reshape(1, 3)
        order = np.argsort(ids, kind="stable")  # (three different points: a triangle that names one twice has no area and is never hit)
        hit["point_ids"], hit["forces"] = ids[order], f[order]
        self.integrator.embed_add_forces(eid, hit["forces"], hit["point_ids"])
        return hit

    def stress(self, world=False, tensors=False):
        """``FemIntegrator.stress``: stress and strain of every element on the device, the summary returned"""
        return self.integrator.stress(world=world, tensors=tensors)

    def element_stress(self, first=0, count=None, tensors=None):
        """``FemIntegrator.element_stress``"""
        return self.integrator.element_stress(first, count, tensors)

    def surface_stress(self):
        """``FemIntegrator.surface_stress``: the per-vertex scalar to draw on ``surface_mesh(update=True)``"""
        return self.integrator.surface_stress()

    def reset_deformations(self):
        self.integrator.reset_to_rest()

    def cut(self, strip, mode="bake"):
        """``FemIntegrator.cut``; the host route's copy of the pattern is dropped with the old mesh"""
        info, delta = self.integrator.cut(strip, mode=mode)
        self.dof, self._pattern = self.integrator.r, None
        return info, delta

    def parts(self):
        """``FemIntegrator.parts``: the disjoint parts of the (cut) body, counted on the device"""
        return self.integrator.parts()

    def split_parts(self, quad, dist):
        """``FemIntegrator.split_parts``: the parts on either side of the quad's plane pushed apart by ``dist`` each"""
        return self.integrator.split_parts(quad, dist)

    def read_part(self, k):
        """``FemIntegrator.read_part``: part ``k`` as a mesh of its own"""
        return self.integrator.read_part(k)

    def _positions(self):
        it = self.integrator
        return np.asarray(it.verts, np.float64).reshape(-1, 3) + it.get_q_state()[0].reshape(-1, 3)

    def pick_vertex(self, wpos):
        """``Deformable::pickVertex`` (Deformable.cpp:422-428): (index, position) of the node of the displaced mesh closest to wpos"""
        if self.haptic_on_device:
            idx, xyz, _ = self.integrator.pick_vertex(wpos)
            return idx, xyz
        p = self._positions()
        d = p - np.asarray(wpos, np.float64)
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        idx = int(np.argmin(d2))  # (the first of equal minima)
        return idx, p[idx].copy()

    def pick_vertices(self, box_lo, box_hi):
        """``Deformable::pickVertices`` (Deformable.cpp:430-448): (positions (k, 3), ascending indices (k,)) inside the box, bounds included"""
        if self.haptic_on_device:
            _, ids, xyz = self.integrator.pick_box(box_lo, box_hi)
            return xyz, ids
        p = self._positions()
        ids = np.nonzero(((p >= np.asarray(box_lo, np.float64)) & (p <= np.asarray(box_hi, np.float64))).all(axis=1))[0].astype(np.int32)
        return p[ids], ids

    def compute_volume(self):
        """``Deformable::computeVolume`` (Deformable.cpp:260-279) at the current state"""
        if self.haptic_on_device:
            return self.integrator.volume()
        p, t = self._positions(), np.asarray(self.integrator.tets)
        u, v, w = p[t[:, 0]] - p[t[:, 3]], p[t[:, 1]] - p[t[:, 3]], p[t[:, 2]] - p[t[:, 3]]
        det = (u[:, 0] * (v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1]) + u[:, 1] * (v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2])) + u[:, 2] * (v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0])
        return float(np.sum(np.abs(det) / 6.0))

    def haptic_start_at(self, wpos):
        """``Deformable::hapticStart(const vec3d&)`` (Deformable.cpp:519-532): picks the node closest to wpos; refuses a clamped one"""
        idx, _ = self.pick_vertex(wpos)
        if idx in self.fixed_vertices:
            return False
        self.haptic_start(idx)
        return True
