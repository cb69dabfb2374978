"""MultiRingNetwork (flow/networks/multi_ring.py): ``num_rings`` separate ring roads in one simulation, ring ``i`` made
of the edges bottom_i -> right_i -> top_i -> left_i.

The rings share nothing but the step counter, so the simulator holds ring ``i`` of environment ``e`` as row
``e * num_rings + i`` of its ``[R, N]`` state (flow_amd.envs.spec.build_spec) and steps every row with the ring kernels.
Each ring gets the four internal edges of 0.1 m that ``RingNetwork`` states for itself (the reference leaves them to
netconvert; no fixture pins their length)."""
from math import pi, sin, cos, ceil, sqrt

import numpy as np

from flow_amd.core.params import InitialConfig, TrafficLightParams
from flow_amd.networks.base import Network

ADDITIONAL_NET_PARAMS = {
    # length of the ring road
    "length": 230,
    # number of lanes
    "lanes": 1,
    # speed limit for all edges
    "speed_limit": 30,
    # resolution of the curves on the ring
    "resolution": 40,
    # number of rings in the system
    "num_rings": 7
}

VEHICLE_LENGTH = 5  # length of vehicles in the network, in meters

RING_EDGES = ("bottom", "right", "top", "left")            # driving order


class MultiRingNetwork(Network):
    """flow/networks/multi_ring.py:24-319."""

    def __init__(self, name, vehicles, net_params, initial_config=InitialConfig(),
                 traffic_lights=TrafficLightParams(), detector_params=None):
        for p in ADDITIONAL_NET_PARAMS.keys():
            if p not in net_params.additional_params:
                raise KeyError('Network parameter "{}" not supplied'.format(p))
        self.length = net_params.additional_params["length"]
        self.lanes = net_params.additional_params["lanes"]
        self.num_rings = net_params.additional_params["num_rings"]
        super().__init__(name, vehicles, net_params, initial_config, traffic_lights, detector_params)

    def specify_edge_starts(self):
        """:78-90: the rings one after the other, no room for the junctions (the reference's table)."""
        edgelen = self.length / 4
        shift = 4 * edgelen
        edgestarts = []
        for i in range(self.num_rings):
            edgestarts += [("bottom_{}".format(i), 0 + i * shift), ("right_{}".format(i), edgelen + i * shift),
                           ("top_{}".format(i), 2 * edgelen + i * shift), ("left_{}".format(i), 3 * edgelen + i * shift)]
        return edgestarts

    @staticmethod
    def gen_custom_start_pos(cls, net_params, initial_config, num_vehicles):
        """:92-148: ``num_vehicles / num_rings`` vehicles per ring; the increment comes from the free length of the
        WHOLE network, so the bunching is shared by the rings.  ``cls`` is the network kernel."""
        min_gap, lanes_distr, available_length, _ = cls._start_pos_util(initial_config, num_vehicles)
        x0 = initial_config.x0
        length = net_params.additional_params["length"]
        num_rings = net_params.additional_params["num_rings"]
        increment = available_length / num_vehicles
        vehs_per_ring = num_vehicles / num_rings

        x = x0
        car_count = 0
        startpositions, startlanes = [], []
        while car_count < num_vehicles:
            pos = cls.get_edge(x)
            # place vehicles side-by-side in all available lanes on this edge
            for lane in range(min(cls.num_lanes(pos[0]), lanes_distr)):
                car_count += 1
                startpositions.append((pos[0], pos[1] % length))
                startlanes.append(lane)
                if car_count == num_vehicles:
                    break
            # 1e-13 prevents an extra car from being added in wrong place
            x = (x + increment + VEHICLE_LENGTH + min_gap) + 1e-13
            if (car_count % vehs_per_ring) == 0:
                # the right number of cars on this ring: move on to the next one
                ring_num = int(car_count / vehs_per_ring)
                x = length * ring_num + 1e-13
        return startpositions, startlanes

    def _centres(self, net_params):
        length = net_params.additional_params["length"]
        ring_num = net_params.additional_params["num_rings"]
        r = length / (2 * pi)
        ring_spacing = 4 * r
        side = int(ceil(sqrt(ring_num)))
        return r, [(j * ring_spacing, k * ring_spacing) for j in range(side) for k in range(side)][:ring_num]

    def specify_nodes(self, net_params):
        r, centres = self._centres(net_params)
        nodes = []
        for i, (cx, cy) in enumerate(centres):
            nodes += [{"id": "bottom_{}".format(i), "x": 0 + cx, "y": -r + cy},
                      {"id": "right_{}".format(i), "x": r + cx, "y": 0 + cy},
                      {"id": "top_{}".format(i), "x": 0 + cx, "y": r + cy},
                      {"id": "left_{}".format(i), "x": -r + cx, "y": 0 + cy}]
        return nodes

    def specify_edges(self, net_params):
        length = net_params.additional_params["length"]
        resolution = net_params.additional_params["resolution"]
        r, centres = self._centres(net_params)
        edgelen = length / 4.
        edges = []
        for i, (cx, cy) in enumerate(centres):
            for q, name in enumerate(RING_EDGES):
                t0 = -pi / 2 + q * pi / 2
                edges.append({"id": "{}_{}".format(name, i), "type": "edgeType", "from": "{}_{}".format(name, i),
                              "to": "{}_{}".format(RING_EDGES[(q + 1) % 4], i), "length": edgelen,
                              "shape": [(r * cos(t) + cx, r * sin(t) + cy) for t in np.linspace(t0, t0 + pi / 2, resolution)]})
        return edges

    def specify_types(self, net_params):
        return [{"id": "edgeType", "numLanes": net_params.additional_params["lanes"],
                 "speed": net_params.additional_params["speed_limit"]}]

    def specify_routes(self, net_params):
        rts = {}
        for i in range(net_params.additional_params["num_rings"]):
            ring = ["{}_{}".format(name, i) for name in RING_EDGES]
            for q in (2, 3, 0, 1):                                       # (the reference's order: top, left, bottom, right)
                rts[ring[q]] = ring[q:] + ring[:q]
        return rts

    def specify_internal_edges(self, junction_length, center_length=None):
        """Per ring what RingNetwork states: one internal edge of ``junction_length`` after every edge."""
        return [(":{}_{}_0".format(RING_EDGES[(q + 1) % 4], i), junction_length)
                for i in range(self.num_rings) for q in range(4)]

    # ---- the simulator's coordinates: ring i is a row, its loop coordinate RingNetwork's (edges and junctions)
    def ring_coordinate(self, edge, position, junction_length=0.1):
        """(ring, loop coordinate on that ring) of a point on ``edge``."""
        name, ring = edge.lstrip(':').split('_')[:2]
        q = RING_EDGES.index(name)
        if edge[0] == ':':                                               # the junction BEFORE edge `name`
            q = (q - 1) % 4
            return int(ring), (q + 1) * 0.25 * self.length + q * junction_length + position
        return int(ring), q * (0.25 * self.length + junction_length) + position

    def ring_locate(self, ring, x, junction_length=0.1):
        """(edge, position on it) of loop coordinate ``x`` of ring ``ring``."""
        span = 0.25 * self.length + junction_length
        q = min(int(x // span), 3)
        u = x - q * span
        if u >= 0.25 * self.length:
            return ":{}_{}_0".format(RING_EDGES[(q + 1) % 4], ring), u - 0.25 * self.length
        return "{}_{}".format(RING_EDGES[q], ring), u
