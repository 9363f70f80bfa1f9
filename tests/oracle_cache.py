"""The float64 / float32 oracle cache shared by tests/mfcc_cases.py and tests/fbank_cases.py: each int16 PCM row goes through
the front end's CPU reference once per precision, and the results are never modified."""
import numpy as np


class OracleCache:
    """reference(x float64 [L] in [-1, 1], dtype, *args) -> [frames, width]; `args` (a sample rate, say) are part of the key"""

    def __init__(self, reference, width):
        self.reference, self.width, self._refs = reference, width, {}

    def refs(self, pcm, *args):
        """(float64 oracle, float32 oracle) [frames, width] of pcm / 32768"""
        key = (pcm.tobytes(),) + args
        if key not in self._refs:
            x = pcm.astype(np.float64) / 32768.0
            r64, r32 = self.reference(x, np.float64, *args), self.reference(x, np.float32, *args)
            r64.setflags(write=False)
            r32.setflags(write=False)
            self._refs[key] = (r64, r32)
        return self._refs[key]

    def e32(self, rows, *args):
        """E32[j]: per output column the largest |float32 oracle - float64 oracle| over every frame of the case's rows"""
        e = np.zeros(self.width)
        for pcm in rows:
            r64, r32 = self.refs(pcm, *args)
            if len(r64):
                e = np.maximum(e, np.abs(r32.astype(np.float64) - r64).max(0))
        return e
