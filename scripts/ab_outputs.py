"""Bit-for-bit comparison of EVERY output of the forward fit between two builds of libdfepe_hip.so, on the training call (pixel matches,
logits in, epi_res + save + weights_out wanted) -- the call whose output phase has a build of its own since round 6 (w8pt16_body.h:
DFEPE_P6_FAST) -- and on the inference call (weights in, no weights_out), for ragged and dropped correspondences.
usage (GPU box): python scripts/ab_outputs.py libA.so libB.so"""
import ctypes, importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
d = importlib.import_module("pytorch-deepfepe_amd")
P, I, U, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_float
libs = []
for path in sys.argv[1:3]:
    L = ctypes.CDLL(os.path.abspath(path))
    L.dfepe_w8pt_fwd.restype = I
    L.dfepe_w8pt_fwd.argtypes = [P, P, P, I, I, I, U, F, F, F, P, P, P, P, P, P]
    libs.append(L)
st = torch.cuda.current_stream().cuda_stream
bad = 0
for B, N in [(4096, 100), (300, 97), (300, 112), (300, 113), (300, 128), (300, 96), (300, 65), (300, 64), (300, 33), (300, 17), (300, 16), (50, 9), (50, 5),
             (40, 129), (20, 1000)]:
    sc = d.synth.make_scene(B, N, seed=3 * N + B, outlier_ratio=0.3, noise_px=0.5)
    m = sc["matches_xy_ori"].clone()
    m[1, N // 2, 2] = float("nan"); m[2, N - 1, 0] = float("inf")
    m = m.cuda().contiguous()
    logits = sc["logits_layers"][0].cuda().contiguous()
    w = torch.softmax(logits, 1).contiguous()
    for flags, wt, want_wout in ((3, logits, True), (1, w, False)):
        outs = []
        for L in libs:
            Fo = torch.full((B, 9), -7.0, device="cuda"); res = torch.full((B, N), -7.0, device="cuda"); epi = torch.full((B, N), -7.0, device="cuda")
            sv = torch.zeros(B, 128, device="cuda"); wo = torch.full((B, N), -7.0, device="cuda")
            rc = L.dfepe_w8pt_fwd(m.data_ptr(), None, wt.data_ptr(), B, N, 1, flags, 1241.0, 376.0, 0.5, Fo.data_ptr(), res.data_ptr(), epi.data_ptr(),
                                  sv.data_ptr(), wo.data_ptr() if want_wout else None, st)
            assert rc == 0, rc
            torch.cuda.synchronize()
            outs.append((Fo, res, epi, sv, wo))
        same = [bool((a.view(torch.int32) == b.view(torch.int32)).all()) for a, b in zip(*outs)]
        print(f"B={B} N={N} flags={flags}: F/residual/epi/save/weights_out bit-identical: {same}")
        bad += not all(same)
print("ALL IDENTICAL" if bad == 0 else f"{bad} MISMATCHES")
