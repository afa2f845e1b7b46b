"""Child of test_gpu_pullback.py, in a process of its own, on the independence case (build()).
  grid OUT : the 1000-point list through pullback_points with whatever TTX_PB_GRID the parent put into the environment; x, logq, val go
             to the .npz OUT
  dev OUT  : the transport helpers on torch tensors on the device (the _dev entries) -- torch brings a HIP runtime of its own and has to
             initialise its device before the engine's library does (tijk_dev_worker.py); pullback_points, transport_sample on the
             reference points, the per-layer round trips and transport_rosenblatt go to the .npz OUT
Prints OK."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(E, P):
    """the layers, reference grid and index list of the independence case (deterministic)"""
    layers = P.make_layers(E, [[5, 17, 9], [9, 4, 6], [3, 7, 5]], [3, [1, 5, 2, 1], 4], [0.0, 0.125, 0.5], seed=40)
    ref = [P.unit_nodes(9), P.unit_nodes(9, seed=3), P.unit_nodes(9)]
    ind = P.random_indices([9, 9, 9], 1000, seed=8)
    return layers, ref, ind


def main():
    what, out = sys.argv[1], sys.argv[2]
    if what == "dev":
        import torch
        torch.cuda.init()
    import pullback_util as P
    from ttcross_amd import engine as E
    layers, ref, ind = build(E, P)
    tt = E.TTCross.pullback(layers, ref, None, 2, pivoting=1)
    x, lq, v = tt.pullback_points(ind)
    if what == "grid":
        np.savez(out, x=x, lq=lq, v=v, grid=os.environ.get("TTX_PB_GRID", ""))
    else:
        u = P.ref_points(ref, ind)
        ud = torch.from_numpy(u).to("cuda:0")
        xs, lqs, vs = E.transport_sample(layers, ud)
        hx, hlq, hv = E.transport_sample(layers, u)                             # host arrays take the same path through the host entries
        per_layer, ut = [], ud
        for y, nodes, g in reversed(layers):                                    # m .. 1: the round trip of each layer at the points the chain feeds it
            xt = y.sample_sq_real(ut, nodes, gamma=g, mode="exact", want=("x",))["x"]
            back = y.rosenblatt_sq_real(xt, nodes, gamma=g, mode="exact", want=("u",))["u"]
            per_layer.append(float((back - ut).abs().max()))
            ut = xt
        ub, lqb, vb = E.transport_rosenblatt(layers, xs)
        np.savez(out, x=x, lq=lq, v=v, u=u, is_cuda=all(bool(t.is_cuda) for t in (xs, lqs, vs, ub, lqb, vb)), xs=xs.cpu().numpy(), lqs=lqs.cpu().numpy(),
                 vs=vs.cpu().numpy(), hx=hx, hlq=hlq, hv=hv, per_layer=np.array(per_layer), ub=ub.cpu().numpy(), lqb=lqb.cpu().numpy(), vb=vb.cpu().numpy())
    tt.close()
    for y, _, _ in layers:
        y.close()
    print("pullback_grid_worker OK")


if __name__ == "__main__":
    main()
