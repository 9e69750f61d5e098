"""
Superpixel graph construction — host mirror of reference src/gcn_grabcut/graph_builder.py.

Same public names (SuperpixelGraphConfig, SuperpixelGraph, GraphBuilder,
compute_auto_prior, encode_user_hints, N_* constants); the arithmetic — colour
conversion, SLIC, region statistics, adjacency and non-local edges, automatic
prior — runs on the MI355X through libggc_hip.so (ggc_preprocess, ggc_slic,
ggc_graph_count / ggc_graph_fill).

Node features (16): mean Lab, std Lab (per-image min-max), mean HSV, centroid y/x,
area ratio, compactness, mean gradient, boundary ratio, centre distance.
Edge features (5): colour distance, centroid distance, shared boundary, gradient
contrast, non-local flag.  Prior (3): fg-ness, bg-ness, ambiguity.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ._constants import N_IMAGE_FEATS, N_PRIOR_FEATS, N_HINT_FEATS, N_NODE_FEATS, N_EDGE_FEATS  # noqa: F401


@dataclass
class SuperpixelGraphConfig:
    """reference graph_builder.py:64-71"""
    n_segments: int = 300       # target superpixel count
    compactness: float = 10.0   # SLIC spatial regularisation
    sigma: float = 1.0          # Gaussian pre-smoothing
    use_lab: bool = True        # SLIC on the Lab image
    connectivity: int = 4       # 4 or 8 — pixel adjacency for edge detection
    n_nonlocal: int = 4         # non-local colour neighbours per node (0 = off)


@dataclass
class SuperpixelGraph:
    """Container for a built superpixel graph (reference graph_builder.py:80-129)."""
    segments: np.ndarray        # (H, W) int32
    node_features: np.ndarray   # (N, 16) float32
    edge_index: np.ndarray      # (2, E) int64, symmetric directed pairs
    edge_attr: np.ndarray       # (E, 5) float32
    n_nodes: int = 0
    n_edges: int = 0
    node_centroids: np.ndarray = field(default_factory=lambda: np.empty((0, 2)))
    prior_features: np.ndarray = field(default_factory=lambda: np.empty((0, N_PRIOR_FEATS)))
    node_areas: np.ndarray = field(default_factory=lambda: np.empty((0,)))

    def node_input(self, prior_features: np.ndarray | None = None) -> np.ndarray:
        """(N, 19) = image features || automatic prior."""
        prior = self.prior_features if prior_features is None else prior_features
        if prior is None or prior.size == 0:
            prior = np.zeros((self.n_nodes, N_PRIOR_FEATS), dtype=np.float32)
        return np.concatenate([self.node_features, prior], axis=1).astype(np.float32)

    def to_networkx(self):
        import networkx as nx
        g = nx.Graph()
        g.add_nodes_from(range(self.n_nodes))
        nx.set_node_attributes(g, {i: self.node_features[i] for i in range(self.n_nodes)}, "feat")
        for i in range(self.edge_index.shape[1]):
            s, d = self.edge_index[0, i], self.edge_index[1, i]
            if s < d:
                g.add_edge(int(s), int(d), attr=self.edge_attr[i])
        return g

    def to_pyg(self, prior_features: np.ndarray | None = None):
        """Graph as this package's Data container (PyG itself is not a dependency)."""
        import torch
        from .data import Data
        area = self.node_areas
        if area is None or area.size == 0:
            area = np.full(self.n_nodes, 1.0 / max(self.n_nodes, 1), dtype=np.float32)
        return Data(
            x=torch.tensor(self.node_input(prior_features), dtype=torch.float32),
            edge_index=torch.tensor(self.edge_index, dtype=torch.long),
            edge_attr=torch.tensor(self.edge_attr, dtype=torch.float32),
            node_area=torch.tensor(area, dtype=torch.float32),
        )


def _check_image(image: np.ndarray) -> np.ndarray:
    if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError("image must be a BGR uint8 array of shape (H, W, 3)")
    return np.ascontiguousarray(image)


def graphs_to_host(graphs, index: int = 0) -> SuperpixelGraph:
    """One image of a DeviceGraphs batch as the reference's host container."""
    n0, n1 = int(graphs.node_ptr_host[index]), int(graphs.node_ptr_host[index + 1])
    e0, e1 = int(graphs.edge_ptr_host[index]), int(graphs.edge_ptr_host[index + 1])
    x = graphs.x[n0:n1].cpu().numpy()
    src = graphs.edge_src[e0:e1].cpu().numpy().astype(np.int64) - n0
    dst = graphs.edge_dst[e0:e1].cpu().numpy().astype(np.int64) - n0
    return SuperpixelGraph(
        segments=graphs.segments[index].cpu().numpy(),
        node_features=np.ascontiguousarray(x[:, :N_IMAGE_FEATS]),
        edge_index=np.stack([src, dst]) if e1 > e0 else np.zeros((2, 0), np.int64),
        edge_attr=graphs.edge_attr[e0:e1].cpu().numpy().reshape(-1, N_EDGE_FEATS),
        n_nodes=n1 - n0,
        n_edges=e1 - e0,
        node_centroids=graphs.centroids[n0:n1].cpu().numpy(),
        prior_features=np.ascontiguousarray(x[:, N_IMAGE_FEATS:]),
        node_areas=graphs.area_ratio[n0:n1].cpu().numpy(),
    )


class GraphBuilder:
    """
    Builds the superpixel adjacency graph of a BGR image on the MI355X
    (reference graph_builder.py:131-175).

        graph = GraphBuilder(image, SuperpixelGraphConfig(n_segments=500)).build()
    """

    def __init__(self, image: np.ndarray, config: SuperpixelGraphConfig | None = None, device="cuda"):
        from ._engine import get_engine
        self.bgr = _check_image(image)
        self.config = config or SuperpixelGraphConfig()
        if self.config.connectivity not in (4, 8):
            raise ValueError("connectivity must be 4 or 8")
        self._eng = get_engine(device)
        self._bgr_d = self._eng.to_device(self.bgr[None])
        # colour prep happens here, like the reference constructor (:142-154)
        self._lab, self._hsv, self._gray, self._grad = self._eng.preprocess(self._bgr_d)

    def build_device(self):
        cfg = self.config
        if cfg.use_lab:
            seg, n = self._eng.slic(self._lab, cfg.n_segments, cfg.compactness, cfg.sigma)
        else:                                      # reference graph_builder.py:177-179: slic(self.rgb.astype(float), ...)
            seg, n = self._eng.slic_rgb(self._bgr_d, cfg.n_segments, cfg.compactness, cfg.sigma)
        return self._eng.build_graphs(seg, n, self._lab, self._hsv, self._grad, cfg.connectivity, cfg.n_nonlocal)

    def build(self) -> SuperpixelGraph:
        return graphs_to_host(self.build_device(), 0)


def compute_auto_prior(segments: np.ndarray, lab: np.ndarray, centre_sigma: float = 0.45,
                       contrast_sigma: float = 0.40, device="cuda") -> np.ndarray:
    """(N, 3) float32 [fg-ness, bg-ness, ambiguity] — reference graph_builder.py:357-444."""
    import torch
    from ._engine import Engine, get_engine
    eng = get_engine(device)
    custom = (float(centre_sigma), float(contrast_sigma)) != (0.45, 0.40)
    if custom:
        # The sigmas are state of a library context.  Non-default values go to a PRIVATE context (one per device, serialised
        # by a lock), so the shared context — which other threads build the pipeline's graphs with — never leaves the defaults.
        with _prior_lock:
            peng = _prior_engines.get(eng.index)
            if peng is None:
                peng = _prior_engines[eng.index] = Engine(eng.index, private_context=True)
            peng.ctx.call("ggc_graph_prior_sigmas", float(centre_sigma), float(contrast_sigma))
            return _auto_prior_on(peng, segments, lab)
    return _auto_prior_on(eng, segments, lab)


_prior_engines: dict = {}
_prior_lock = __import__("threading").Lock()


def _auto_prior_on(eng, segments: np.ndarray, lab: np.ndarray) -> np.ndarray:
    import torch
    seg = eng.to_device(np.ascontiguousarray(segments, dtype=np.int32)[None])
    lab_d = eng.to_device(np.ascontiguousarray(lab, dtype=np.float32)[None])
    h, w = segments.shape
    n = torch.tensor([int(segments.max()) + 1], dtype=torch.int32, device=eng.device)
    zeros3 = torch.zeros(1, h, w, 3, device=eng.device)
    zeros1 = torch.zeros(1, h, w, device=eng.device)
    graphs = eng.build_graphs(seg, n, lab_d, zeros3, zeros1, 4, 0)
    return graphs.x[:, N_IMAGE_FEATS:].cpu().numpy()


def encode_user_hints(segments: np.ndarray, fg_points, bg_points) -> np.ndarray:
    """Legacy click features (reference graph_builder.py:457-494); a host-side
    table lookup that the automatic pipeline never calls."""
    n_nodes = int(segments.max()) + 1
    hints = np.zeros((n_nodes, 3), dtype=np.float32)
    hints[:, 2] = 1.0
    for col, points in ((0, fg_points), (1, bg_points)):
        for r, c in points:
            r, c = int(r), int(c)
            if 0 <= r < segments.shape[0] and 0 <= c < segments.shape[1]:
                nid = int(segments[r, c])
                hints[nid, col] = 1.0
                hints[nid, 2] = 0.0
    return hints


def geodesic_prior_columns(node_dist: np.ndarray, radius: int, sigma: float) -> np.ndarray:
    """(N,2) int32 capped per-superpixel distances (min Df, min Db) -> (N,3) float32 soft click columns: e_f =
    exp(-Df / (80 sigma)), 0 where Df is the cap 80 radius + 1 (no foreground click within reach), e_b likewise, and
    1 - max(e_f, e_b).  Computed in float64, cast to float32."""
    nd = np.asarray(node_dist, np.float64).reshape(-1, 2)
    e = np.where(nd > 80 * int(radius), 0.0, np.exp(-nd / (80.0 * float(sigma))))
    return np.concatenate([e, 1.0 - e.max(axis=1, keepdims=True)], 1).astype(np.float32)


def encode_geodesic_hints(image: np.ndarray, segments: np.ndarray, fg_points, bg_points, geodesic=None,
                          device="cuda") -> np.ndarray:
    """Soft click features (additive): the reference paper's "soft distance-based propagation (geodesic
    distance to the nearest click)" in place of encode_user_hints' binary columns.  image: (H, W, 3) uint8 BGR;
    segments: (H, W) labels 0..n-1; geodesic: a pipeline.GeodesicHints (None: its defaults).  Row n is (e_f, e_b,
    1 - max(e_f, e_b)) with e = exp(-D_n / (80 sigma)), D_n the smallest geodesic distance from a pixel of superpixel n
    to a click of that label (ggc_geodesic_hints' node_dist), and e = 0 beyond the cap.  Without a click in the frame
    every row is (0, 0, 1), as encode_user_hints gives.  No shipped network was trained on this encoding: it is what
    segment(..., hints_as_prior=True, geodesic=...) feeds the network, offered for training such a network."""
    import torch
    from ._engine import get_engine
    from .pipeline import GeodesicHints
    g = GeodesicHints() if geodesic is None or geodesic is True else geodesic
    if not isinstance(g, GeodesicHints):
        raise ValueError(f"geodesic must be a GeodesicHints, got {type(geodesic).__name__}")
    img = _check_image(image)
    seg = np.ascontiguousarray(segments, np.int32)
    if seg.shape != img.shape[:2]:
        raise ValueError(f"segments {seg.shape} do not match the image {img.shape[:2]}")
    n = int(seg.max()) + 1
    rows, ptr = pack_hints([(fg_points if fg_points is not None else [], bg_points if bg_points is not None else [])])
    if len(rows) == 0:
        return geodesic_prior_columns(np.full((n, 2), 80 * g.radius + 1, np.int32), g.radius, g.sigma)
    eng = get_engine(device)
    hint_rows, hint_ptr = eng.upload_hints(rows, ptr)
    nd = eng.empty(n, 2, dtype=torch.int32)
    eng.geodesic_hints(eng.to_device(img[None]), hint_rows, hint_ptr, g.radius, g.gamma, segments=eng.to_device(seg[None]),
                       node_ptr=eng.to_device(np.array([0, n], np.int32)), node_dist=nd)
    return geodesic_prior_columns(nd.cpu().numpy(), g.radius, g.sigma)


def _click_rows(points, label: int, what: str) -> np.ndarray:
    a = np.asarray(list(points) if points is not None else [], dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 3), np.int64)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what} must be a sequence of (row, col) pairs, got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} holds a non-finite coordinate")
    rc = np.trunc(a).astype(np.int64)                         # int(r), int(c) as in encode_user_hints
    if (np.abs(rc) > np.iinfo(np.int32).max).any():
        raise ValueError(f"{what} holds a coordinate outside the int32 range")
    return np.concatenate([rc, np.full((len(rc), 1), label, np.int64)], 1)


def _check_entry(entry, n: int, what: str, parts: str) -> None:
    """One image's entry of a pack_* call: a sequence of n parts."""
    if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__") or len(entry) != n:
        raise ValueError(f"{what} must be None or a {parts}")


def _pack_rows(per_image, name: str, items: str, rows_of, width: int, counted: str) -> "tuple[np.ndarray, np.ndarray]":
    """What pack_hints and pack_strokes share: per image None or a (foreground, background) pair -> (rows int32 [n,width],
    ptr int32 [B+1]), an image's foreground rows before its background rows.  rows_of(part, label, what) -> int64 [m,width]."""
    rows, ptr = [], [0]
    for b, entry in enumerate(per_image):
        n = 0
        if entry is not None:
            _check_entry(entry, 2, f"{name}[{b}]", f"(fg_{items}, bg_{items}) pair")
            for part, label, ground in ((entry[0], 1, "foreground"), (entry[1], 0, "background")):
                rows.append(rows_of(part, label, f"{name}[{b}] {ground} {items}"))
                n += len(rows[-1])
        ptr.append(ptr[-1] + n)
    if ptr[-1] > np.iinfo(np.int32).max // width:
        raise ValueError(f"{ptr[-1]} {counted}: too many for one call")
    packed = np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, width), np.int32)
    return np.ascontiguousarray(packed.reshape(-1, width)), np.asarray(ptr, np.int32)


def pack_hints(per_image) -> "tuple[np.ndarray, np.ndarray]":
    """Per-image click lists -> the (hints, hint_ptr) pair of ggc_apply_hints.

    per_image: one entry per image, None (no clicks) or (fg_points, bg_points), each a sequence of (row, col) as in
    encode_user_hints.  Returns hints int32 [K,3] = (row, col, label) with label 1 = foreground, 0 = background, and
    hint_ptr int32 [B+1].  An image's foreground clicks come first, then its background clicks, each in the order given,
    so a background disk wins where the two overlap.  Clicks outside the image are kept: the kernel ignores them."""
    return _pack_rows(per_image, "hints", "points", _click_rows, 3, "clicks")


STROKE_MAX_COORD = 1 << 20          # ggc_apply_strokes' limit on an endpoint coordinate


def _stroke_segments(strokes, label: int, what: str) -> np.ndarray:
    """The polylines of one label -> their segments, int64 [n,5] = (r0, c0, r1, c1, label)."""
    out = []
    if strokes is None:
        return np.zeros((0, 5), np.int64)
    if isinstance(strokes, (str, bytes)):
        raise ValueError(f"{what} must be a sequence of strokes, each a sequence of (row, col) vertices")
    for i, stroke in enumerate(strokes):
        v = _click_rows(stroke, label, f"{what}[{i}]")[:, :2] if not isinstance(stroke, (str, bytes)) else None
        if v is None or len(v) == 0:
            raise ValueError(f"{what}[{i}] is empty: a stroke has at least one (row, col) vertex")
        if (np.abs(v) > STROKE_MAX_COORD).any():
            raise ValueError(f"{what}[{i}] holds a coordinate beyond +-2^20")
        a, b = (v, v) if len(v) == 1 else (v[:-1], v[1:])
        out.append(np.concatenate([a, b, np.full((len(a), 1), label, np.int64)], 1))
    return np.concatenate(out) if out else np.zeros((0, 5), np.int64)


def pack_strokes(per_image) -> "tuple[np.ndarray, np.ndarray]":
    """Per-image brush strokes -> the (strokes, stroke_ptr) pair of ggc_apply_strokes; the sibling of pack_hints.

    per_image: one entry per image, None (no strokes) or (fg_strokes, bg_strokes), each a sequence of strokes, a stroke
    being a sequence of (row, col) vertices: a polyline of n >= 2 vertices gives n-1 segments, a one-vertex stroke one
    segment with both ends equal.  Returns strokes int32 [S,5] = (r0, c0, r1, c1, label) with label 1 = foreground,
    0 = background, and stroke_ptr int32 [B+1].  An image's foreground strokes come first, then its background strokes,
    each in the order given, so background wins where the two overlap.  Vertices outside the image are kept: the kernel
    paints the part of a segment that lies inside.  An empty stroke, a wrong shape or a coordinate beyond +-2^20 is a
    ValueError."""
    return _pack_rows(per_image, "strokes", "strokes", _stroke_segments, 5, "stroke segments")


def scissors_list(scissors) -> list:
    """The `scissors` argument of the public calls, one anchor list or a sequence of them (or None) -> a list of anchor lists."""
    if scissors is None:
        return []
    if isinstance(scissors, (str, bytes)):
        raise ValueError("scissors must be a sequence of (row, col) anchors, or a sequence of such sequences")
    return [scissors] if _is_polygon(scissors) else list(scissors)


def pack_paths(per_image, closed: bool = True) -> "tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]":
    """Per-image anchor paths -> the (anchors, path_ptr, path_closed, image_ptr) arrays of ggc_trace_paths (include/ggc.h
    H4); the sibling of pack_hints.

    per_image: one entry per image, None (no paths) or a sequence of paths.  A path is a sequence of (row, col) anchors,
    closed or open as `closed` says, or an (anchors, closed) pair with its own bool.  Returns anchors int32 [A,2], path_ptr
    int32 [Q+1], path_closed int32 [Q] and image_ptr int32 [B+1].  An open path of fewer than 2 anchors, a closed one of
    fewer than 3 or a wrong shape is a ValueError; whether an anchor lies inside its image is checked by the call."""
    anchors, path_ptr, flags, image_ptr = [], [0], [], [0]
    for b, entry in enumerate(per_image):
        if entry is not None:
            if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__"):
                raise ValueError(f"paths[{b}] must be None or a sequence of paths")
            for i, path in enumerate(entry):
                what, c = f"paths[{b}][{i}]", bool(closed)
                if isinstance(path, tuple) and len(path) == 2 and isinstance(path[1], (bool, np.bool_)):
                    path, c = path[0], bool(path[1])
                if isinstance(path, (str, bytes)):
                    raise ValueError(f"{what} must be a sequence of (row, col) anchors")
                v = _click_rows(path, 0, what)[:, :2]
                if len(v) < (3 if c else 2):
                    raise ValueError(f"{what} has {len(v)} anchors: {'a closed path needs at least 3' if c else 'an open path needs at least 2'}")
                anchors.append(v)
                path_ptr.append(path_ptr[-1] + len(v))
                flags.append(int(c))
        image_ptr.append(len(flags))
    if path_ptr[-1] > np.iinfo(np.int32).max // 2:
        raise ValueError(f"{path_ptr[-1]} anchors: too many for one call")
    a = np.concatenate(anchors).astype(np.int32) if anchors else np.zeros((0, 2), np.int32)
    return (np.ascontiguousarray(a.reshape(-1, 2)), np.asarray(path_ptr, np.int32), np.asarray(flags, np.int32),
            np.asarray(image_ptr, np.int32))


POLYGON_MAX_COORD = 1 << 20         # ggc_apply_polygons' limit on a vertex coordinate
POLYGON_BG, POLYGON_FG, POLYGON_LASSO = 0, 1, 2


def _is_polygon(obj) -> bool:
    """True for one polygon, a sequence of (row, col) pairs; False for a sequence of polygons (or anything else)."""
    try:
        a = np.asarray(obj, dtype=np.float64)
    except (TypeError, ValueError):
        return False
    return a.ndim == 2 and a.shape[1] == 2


def lasso_list(lasso) -> list:
    """The `lasso` argument of the public calls, one polygon or a sequence of polygons (or None) -> a list of polygons."""
    if lasso is None:
        return []
    if isinstance(lasso, (str, bytes)):
        raise ValueError("lasso must be a polygon, a sequence of (row, col) vertices, or a sequence of polygons")
    return [lasso] if _is_polygon(lasso) else list(lasso)


def _polygon_rows(polygons, what: str) -> "list[np.ndarray]":
    """The polygons of one label -> their vertices, one int64 [n,2] array each."""
    if polygons is None:
        return []
    if isinstance(polygons, (str, bytes)):
        raise ValueError(f"{what} must be a sequence of polygons, each a sequence of (row, col) vertices")
    out = []
    for i, poly in enumerate(polygons):
        if isinstance(poly, (str, bytes)):
            raise ValueError(f"{what}[{i}] must be a sequence of (row, col) vertices")
        v = _click_rows(poly, 0, f"{what}[{i}]")[:, :2]
        if len(v) < 3:
            raise ValueError(f"{what}[{i}] has {len(v)} vertices: a polygon has at least 3")
        if (np.abs(v) > POLYGON_MAX_COORD).any():
            raise ValueError(f"{what}[{i}] holds a coordinate beyond +-2^20")
        out.append(v)
    return out


def pack_polygons(per_image) -> "tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]":
    """Per-image polygons -> the (verts, poly_ptr, poly_label, image_ptr) arrays of ggc_apply_polygons; the sibling of
    pack_strokes.

    per_image: one entry per image, None (no polygons) or (fg_polygons, bg_polygons, lassos), each a sequence of polygons,
    a polygon being a sequence of n >= 3 (row, col) vertices, closed implicitly from the last to the first.  Returns verts
    int32 [V,2], poly_ptr int32 [P+1], poly_label int32 [P] (0 = background fill, 1 = foreground fill, 2 = lasso) and
    image_ptr int32 [B+1].  An image's lassos come first, then its foreground fills, then its background fills, each in
    the order given, so background wins where fills overlap, as with clicks and strokes.  Vertices outside the image are
    kept.  A polygon of fewer than 3 vertices, a wrong shape or a coordinate beyond +-2^20 is a ValueError."""
    verts, poly_ptr, labels, image_ptr = [], [0], [], [0]
    for b, entry in enumerate(per_image):
        if entry is not None:
            _check_entry(entry, 3, f"polygons[{b}]", "(fg_polygons, bg_polygons, lassos) triple")
            for polys, label, what in ((entry[2], POLYGON_LASSO, "lassos"), (entry[0], POLYGON_FG, "foreground polygons"),
                                       (entry[1], POLYGON_BG, "background polygons")):
                for v in _polygon_rows(polys, f"polygons[{b}] {what}"):
                    verts.append(v)
                    poly_ptr.append(poly_ptr[-1] + len(v))
                    labels.append(label)
        image_ptr.append(len(labels))
    if poly_ptr[-1] > np.iinfo(np.int32).max // 2:
        raise ValueError(f"{poly_ptr[-1]} polygon vertices: too many for one call")
    v = np.concatenate(verts).astype(np.int32) if verts else np.zeros((0, 2), np.int32)
    return (np.ascontiguousarray(v.reshape(-1, 2)), np.asarray(poly_ptr, np.int32), np.asarray(labels, np.int32),
            np.asarray(image_ptr, np.int32))
