"""Reader of tests/golden/refcfg.npz (tests/golden/make_golden_refcfg.py: the reference's whole model at depth 5, N = 1000 / 2000, in
float64, plus the distances of its own float32 run) and the distance metrics the generator states, shared by tests/test_refcfg_cpu.py
and tests/test_refcfg_gpu.py.  Test infrastructure only."""
import numpy as np
import torch

IMAGE_SIZE = [376, 1241, 3]
DEPTH = 5
CASES = {"n1000": (4, 1000), "n2000": (2, 2000)}
SCENE_KEYS = ("matches_xy_ori", "Ks", "delta_Rtijs_4_4", "qs_cam", "ts_cam", "pts1_virt_ori", "pts2_virt_ori")
LOSS_PARAMS = {"depth": DEPTH, "clamp_at": 0.02, "if_tri_depth": False, "if_sample_loss": False, "topK": 8, "matches_good_unique_nums": None}
FLOOR = 1e-6  # of the largest entry of a quantity's truth: ~16 float32 ulps, below which no fp32 evaluation can be told from another
FACTOR = 4.0  # two independent fp32 evaluations of one function (sqrt 2) x a maximum over 1e4 - 1e6 entries (~2)


class Fixture:
    def __init__(self, z):
        self.z = z

    def __contains__(self, key):
        return key in self.z.files or key + "__planes" in self.z.files

    def __getitem__(self, key):
        """Large float arrays are stored as byte planes (make_golden_refcfg.put); this is its exact inverse."""
        if key + "__planes" in self.z.files:
            planes = self.z[key + "__planes"]
            dt = {4: np.float32, 8: np.float64}[planes.shape[0]]
            return np.ascontiguousarray(planes.T).reshape(-1).view(dt).reshape(tuple(self.z[key + "__shape"]))
        return self.z[key]

    def t(self, key):
        """float64 torch tensor"""
        return torch.from_numpy(np.asarray(self[key], dtype=np.float64))

    def weights(self, case):
        """The truth's weights: softmax over the points of the stored float64 logits (deepFEPE/models/DeepFNet.py:443,512)."""
        return torch.softmax(self.t(case + "_logits_layers"), dim=2)

    def small(self):
        return [str(s) for s in self.z["small"]]


def directions(dir_seed, i, numel):
    """The 4 seeded Gaussian directions of the parameter of index i in the sorted names (recipe of make_golden_refcfg.py)."""
    return torch.stack([torch.randn(numel, generator=torch.Generator().manual_seed(int(dir_seed) * 1000003 + 4 * i + k), dtype=torch.float64)
                        for k in range(4)])


def build_cpu_params(net, synth, param_seed, head):
    """The fixture's parameters: seeded fill of the float32 module, then the last conv of both estimators times ``head`` (on the CPU, in
    float32: one IEEE multiplication per element, the same bits everywhere)."""
    synth.fill_params_deterministic(net, seed=int(param_seed))
    with torch.no_grad():
        for est in (net.input_weights, net.update_weights):
            est.fw[-1].weight.mul_(float(head))
    return net


def unit(F):
    return F / F.flatten(-2).norm(dim=-1)[..., None, None]


def unit_f_dist(a, t):
    """[L,B,3,3] x 2 -> [L]: max over the pairs of the Frobenius distance of the unit-norm F (``a`` in the gauge of ``t``)."""
    return (unit(a) - unit(t)).flatten(2).norm(dim=2).max(1)[0]


def grad_denominators(norms64):
    """max(|g64|, 1e-3 largest |g64|) per parameter: the denominator of the generator's gradient distance."""
    n = torch.as_tensor(norms64, dtype=torch.float64)
    return torch.maximum(n, 1e-3 * n.max())


def bound(ref32_dist, truth_max):
    return max(FACTOR * float(ref32_dist), FLOOR * float(truth_max))
