"""Host reference of od_net_refresh (include/odhip.h): what the loader computes for one layer -- net.pack_layer of
weights.fold_bn -- applied to arrays cut out of a trainer's flat buffers, including the "#split" pack ([w | w] along
the input channels) and the image layer ([Cout, 32] pack, scale additionally divided by 255).  Nothing of its own: the
two functions it calls are the ones Net.__init__ calls, so "equal to this reference" is "equal to the host route".
"""
import numpy as np

from object_detector_amd import net as N
from object_detector_amd import weights as W


def entry(w_offset, cout, cin, ksize, cin_repeat=1, first=False, gamma=None, beta=None, mean=None, var=None, bias=None):
    """One table entry as a dict: the fields of od_refresh_layer that do not depend on device pointers.  BatchNorm layers
    give gamma / beta offsets (parameter buffer) and mean / var offsets (statistics buffer); the others give bias."""
    has_bn = bias is None
    if first:
        cout_pad, kpad = cout, 32
    else:
        cout_pad, kpad = -(-cout // 256) * 256, -(-(ksize * ksize * cin * cin_repeat) // 64) * 64
    return dict(w_offset=w_offset, gamma_offset=gamma if has_bn else 0, beta_offset=beta if has_bn else bias,
                mean_offset=mean if has_bn else 0, var_offset=var if has_bn else 0, Cout=cout, Cin=cin, ksize=ksize,
                Cout_pad=cout_pad, Kpad=kpad, cin_repeat=cin_repeat, first=int(first), has_bn=int(has_bn))


def layer_ref(params_flat, stats_flat, e, eps=W.BN_EPS):
    """-> (pack f16 [Cout_pad, Kpad], scale f32 [Cout_pad], bias f32 [Cout_pad]) of entry `e`."""
    assert np.float32(eps) == np.float32(W.BN_EPS)  # fold_bn's constant
    cout, cin, k = e["Cout"], e["Cin"], e["ksize"]
    w = np.asarray(params_flat[e["w_offset"]:e["w_offset"] + cout * k * k * cin], np.float32).reshape(cout, k, k, cin)
    p = {"l.w": w}
    if e["has_bn"]:
        p["l.gamma"] = params_flat[e["gamma_offset"]:e["gamma_offset"] + cout]
        p["l.beta"] = params_flat[e["beta_offset"]:e["beta_offset"] + cout]
        p["l.mean"] = stats_flat[e["mean_offset"]:e["mean_offset"] + cout]
        p["l.var"] = stats_flat[e["var_offset"]:e["var_offset"] + cout]
    else:
        p["l.bias"] = params_flat[e["beta_offset"]:e["beta_offset"] + cout]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        scale, bias = W.fold_bn(p, "l")
        if e["first"]:
            scale = (scale / np.float32(255.0)).astype(np.float32)  # Net.__init__'s uint8 normalisation
        if e["cin_repeat"] == 2:
            w = np.concatenate([w, w], axis=3)  # Net.__init__'s "#split" operand
        wp, scale, bias = N.pack_layer(w, scale, bias, bool(e["first"]))
    assert wp.shape == (e["Cout_pad"], e["Kpad"]) and scale.shape == bias.shape == (e["Cout_pad"],)
    return wp, scale, bias


class FakeTrainer:
    """The attributes of a Trainer that the table builder and the argument checks read, laid out by Trainer.__init__'s own
    rule (segments padded to 4 elements, (mean, var) pairs in one statistics buffer), with no device behind them."""

    def __init__(self, num_classes=20, neck_ch=256, tower=1, device="cuda:0", ema_decay=None):
        import torch
        from object_detector_amd import desc
        self.num_classes, self.neck_ch, self.tower = num_classes, neck_ch, tower
        self.device, self.ema_decay, self.steps_issued = torch.device(device), ema_decay, 0
        self.specs = {s[0]: s for s in W.layer_specs(num_classes, neck_ch, tower)}
        self.seg, off = {}, 0
        for name, (_n, cin, cout, k, _s, bn) in self.specs.items():
            for kind, n in (("w", cout * k * k * cin),) + ((("gamma", cout), ("beta", cout)) if bn else (("bias", cout),)):
                self.seg[(name, kind)] = (off, n)
                off += desc.pad_to(n, 4)
        self.n_flat = off
        self._run_off, roff = {}, 0
        for n, sp in self.specs.items():
            if sp[5]:
                self._run_off[n] = roff
                roff += 2 * desc.pad_to(sp[2], 4)
        self.n_stats = roff

    def flat_from(self, params):
        """(params_flat, stats_flat) holding an export_params-shaped dict."""
        from object_detector_amd import desc
        flat, stats = np.zeros(self.n_flat, np.float32), np.zeros(self.n_stats, np.float32)
        for (name, kind), (o, n) in self.seg.items():
            flat[o:o + n] = np.asarray(params[f"{name}.{kind}"], np.float32).reshape(-1)
        for name, o in self._run_off.items():
            c = self.specs[name][2]
            stats[o:o + c] = params[name + ".mean"]
            stats[o + desc.pad_to(c, 4):o + desc.pad_to(c, 4) + c] = params[name + ".var"]
        return flat, stats
