"""The helpers every operation used to carry under its own prefix have one definition each (no GPU): the wave reductions, clip8, the
partial quad store and the NaN-first min / max in csrc/device_common.h; the host/device qualifier, the failure macro, the alignment
test and the layout rounding in csrc/check_common.h.  Calls, not copies: the sources are read, nothing is compiled (the *_host tests
build tools/*_check.cpp with a host compiler, which is what proves check_common.h plain C++)."""
import glob
import os
import re

import makefile_rules

CSRC = makefile_rules.CSRC
DEVICE, CHECK = 'device_common.h', 'check_common.h'
SOURCES = {os.path.basename(p): open(p).read() for ext in ('*.hip', '*.h') for p in glob.glob(os.path.join(CSRC, ext))}
# a function whose first statement is the xor butterfly over the offsets 32, 16, .., 1
BUTTERFLY = r'__device__[^\n;{]*\b(\w+)\([^)]*\)\s*\{\s*(?:#pragma unroll\s*)?for \(int (\w+) = 32; \2 > 0; \2 >>= 1\)[^\n]*__shfl_xor'
BUTTERFLY_BLOCK = r'__device__[^\n;{]*\b(\w+)\([^)]*\)\s*\{\s*(?:#pragma unroll\s*)?for \(int (\w+) = 32; \2 > 0; \2 >>= 1\) \{\s*[^\n]*__shfl_xor'


def definitions(pattern):
    """(file, name) of every match of `pattern`, whose first group is the defined name"""
    return sorted((name, m.group(1)) for name, text in SOURCES.items() for m in re.finditer(pattern, text))


def test_the_sources_are_all_there():
    assert DEVICE in SOURCES and CHECK in SOURCES and len([n for n in SOURCES if n.endswith('.hip')]) >= 46
    assert len([n for n in SOURCES if n.endswith('_check.h')]) >= 14


def test_the_wave_reductions_are_defined_once_in_the_device_header():
    found = definitions(BUTTERFLY) + definitions(BUTTERFLY_BLOCK)
    assert sorted(found) == [(DEVICE, 'wave_fmaxf'), (DEVICE, 'wave_fminf'), (DEVICE, 'wave_imax'), (DEVICE, 'wave_imin'),
                             (DEVICE, 'wave_max_greater'), (DEVICE, 'wave_sum')]
    assert definitions(r'__device__[^\n;{]*\b(\w*wave_exclusive_sum|\w*wave_before)\(') == [(DEVICE, 'wave_exclusive_sum')]
    dev = SOURCES[DEVICE]
    # every reduction walks 32, 16, .., 1: a floating-point sum keeps its bits
    assert len(re.findall(r'for \(int o = 32; o > 0; o >>= 1\)', dev)) == 6 and not re.search(r'for \(int \w+ = 1; \w+ < 64', dev.split('wave_exclusive_sum')[0])
    # the three NaN rules stay apart, each under its own name
    body = {n: dev[dev.index(n + '('):].split('\n}\n')[0] for n in ('wave_sum', 'wave_imin', 'wave_imax', 'wave_fminf', 'wave_fmaxf', 'wave_max_greater')}
    assert 'fminf(v, __shfl_xor(v, o, 64))' in body['wave_fminf'] and 'fmaxf(v, __shfl_xor(v, o, 64))' in body['wave_fmaxf']
    assert 'v = t > v ? t : v;' in body['wave_max_greater'] and 'fmax' not in body['wave_max_greater']
    assert 'v = min(v, __shfl_xor(v, o, 64))' in body['wave_imin'] and 'v = max(v, __shfl_xor(v, o, 64))' in body['wave_imax']
    assert 'v += __shfl_xor(v, o, 64)' in body['wave_sum'] and 'template <typename T>\n__device__ __forceinline__ T wave_sum(T v)' in dev
    # and they are called where the copies were
    for name, calls in (('mrcnn_loss.hip', ('wave_sum(', 'wave_max_greater(', 'wave_exclusive_sum(')), ('segm_loss.hip', ('wave_sum(',)),
                        ('segm_tail.hip', ('wave_sum(',)), ('encode_input.hip', ('wave_sum(',)), ('train_items_common.h', ('wave_sum(',)),
                        ('train_items.hip', ('wave_sum(', 'wave_imin(', 'wave_imax(')), ('scene_ids.hip', ('wave_imin(', 'wave_imax(')),
                        ('scene_masks.hip', ('wave_fminf(', 'wave_fmaxf(', 'wave_sum(', 'wave_imin(', 'wave_imax(')),
                        ('fast_segment.hip', ('wave_sum(',)), ('rank_select.h', ('wave_exclusive_sum(',))):
        for call in calls:
            assert call in SOURCES[name], (name, call)
    assert '__shfl_up' not in SOURCES['rank_select.h'] and '__shfl_up' not in SOURCES['mrcnn_loss.hip']   # the one scan is the shared one


def test_clip8_the_quad_store_and_the_nan_first_pair_are_defined_once_in_the_device_header():
    assert definitions(r'__device__[^\n;{]*\b(\w*clip8)\(int \w+\)\s*\{') == [(DEVICE, 'clip8')]
    assert definitions(r'__device__[^\n;{]*\b(\w*store_quad)\([^)]*\)\s*\{') == [(DEVICE, 'store_quad')]
    dev = SOURCES[DEVICE]
    assert 'struct Quad<float> { using type = float4; }' in dev and 'struct Quad<uint32_t> { using type = uint4; }' in dev
    # the rule itself, whatever the function is called: a NaN on either side is the result
    rule = r'\b(\w+)\((\w+) a, \2 b\) \{ return \(a [<>] b \|\| a != a\) \? a : b; \}'
    assert definitions(rule) == [(DEVICE, 'nan_first_max'), (DEVICE, 'nan_first_min')]
    assert '(a > b || a != a) ? a : b' in dev and '(a < b || a != a) ? a : b' in dev
    for name in ('detection_targets.hip', 'rpn_targets.hip'):
        assert 'nan_first_max(' in SOURCES[name] and 'nan_first_min(' in SOURCES[name] and '#include "device_common.h"' in SOURCES[name]
    for name in ('scene_crops.hip', 'scene_paint2d.hip', 'scene_masks.hip', 'assemble.hip', 'raster_composite.hip', 'train_items_common.h'):
        assert re.search(r'(?<!\w)clip8\(', SOURCES[name]), name
    assert 'store_quad(' in SOURCES['scene_masks.hip'] and 'store_quad(' in SOURCES['scene_ids.hip']


def test_the_check_headers_share_one_macro_pair_one_alignment_test_and_one_rounding():
    assert definitions(r'#define (\w+_FAIL)\b') == [(CHECK, 'SDN_FAIL')]
    # SDN_TL_HD carries no __forceinline__ and stays where it is (train_loss_index.h); each macro has its HIP and its host form
    assert definitions(r'#define (\w+_HD)\b') == [(CHECK, 'SDN_HD')] * 2 + [('train_loss_index.h', 'SDN_TL_HD')] * 2
    assert definitions(r'\b(\w*misaligned)\(const void\*[^)]*\)\s*\{') == [(CHECK, 'misaligned')]
    assert definitions(r'\bsize_t (\w*round\w*)\(size_t[^)]*\)\s*\{') == [(CHECK, 'round_up')]
    chk = SOURCES[CHECK]
    assert '#define SDN_HD __host__ __device__ __forceinline__' in chk and '#define SDN_HD inline' in chk
    assert re.search(r'#define SDN_FAIL\(\.\.\.\)\s*\\\n\s*do \{\s*\\\n\s*std::snprintf\(msg, cap, __VA_ARGS__\);\s*\\\n\s*return 1;\s*\\\n\s*\} while \(0\)', chk)
    # no header includes another operation's for a macro: the comments that said so are gone, and the two headers that borrowed
    # segm_tail_check.h's pair and nothing else include the common one alone
    assert not [name for name, text in SOURCES.items() if re.search(r'#include "\w+"\s*//[^\n]*_(HD|FAIL)\b', text)]
    for name in ('encode_input_check.h', 'segm_ppm_check.h'):
        assert re.findall(r'#include "([^"]+)"', SOURCES[name]) == [CHECK], name
    for name, text in SOURCES.items():
        if name.endswith('_check.h'):
            assert CHECK in reach(name), name


def test_the_device_loaders_hold_one_copy_of_the_select_the_debug_count_and_the_pillow_bodies():
    everything = ''.join(SOURCES.values())
    # one switch, one host helper around a counting kernel, used by the three entry points that state a precondition
    assert everything.count('getenv("SDN_DEBUG_CHECKS")') == 1 and 'getenv("SDN_DEBUG_CHECKS")' in SOURCES['sdn_common.h']
    assert everything.count('hipFree(flag)') == 1
    for name, calls in (('scene_crops.hip', 1), ('scene_ids.hip', 2)):
        assert SOURCES[name].count('debug_count("sdn_') == calls and 'debug_checks()' in SOURCES[name], name
    # the jitter is read from the item rows themselves: nothing fills a TrainItem field by field
    assert 'j.frame = 0' not in everything and not re.search(r'\bTrainItem \w+jitter\w*\(', everything)
    assert 'template <class Item>\n__device__ __forceinline__ void ti_jitter(const Item& it,' in SOURCES['train_items_common.h']
    # the radix select calls the rank search from exactly one select kernel and one pick kernel, and both entry points launch those
    loaders = {name: SOURCES[name] for name in ('scene_ids.hip', 'train_hybrid.hip', 'train_items.hip', 'segm_train.hip', 'training_item.hip')}
    callers = sorted((name, kernel) for name, text in loaders.items() for kernel, body in kernels(text) if 'ids_find(' in body)
    assert callers == [('scene_ids.hip', 'k_ids_pick'), ('scene_ids.hip', 'k_ids_select')]
    assert sum(text.count('ids_find(') for text in loaders.values()) == 4   # two ranks in each
    assert not re.search(r'\bk_tid_(init|select|pick)\b', everything)
    assert len(re.findall(r'return ids_chain\(', SOURCES['scene_ids.hip'])) == 2
    # the packed colour of a scene pixel and the accumulation of a Pillow pass are each written once
    assert everything.count('| ((int)s[1] << 8) |') == 1 and 'code24(const uint8_t* s)' in SOURCES[DEVICE]
    for name in ('train_items_common.h', 'train_items.hip', 'train_hybrid.hip', 'segm_train.hip', 'segm_tail.hip'):
        assert 'code24(' in reach_text(name), name
    common = SOURCES['train_items_common.h']
    assert len(re.findall(r'int acc = 1 << \(TI_BITS - 1\)', everything)) == 1 and len(re.findall(r'acc >> TI_BITS', everything)) == 1
    assert common.index('int acc = 1 << (TI_BITS - 1)') < common.index('ti_resample_byte(', common.index('ti_crops_body('))
    # one luma partial and one band body, called by the two image loaders
    for name, calls in (('segm_train.hip', ('ti_luma_body(', 'ti_band_body(')), ('training_item.hip', ('ti_luma_body(', 'ti_band_body('))):
        for call in calls:
            assert SOURCES[name].count(call) == 1, (name, call)
        assert 'ti_jitter(' not in SOURCES[name] and 'SRC_PIXELS + i] =' not in SOURCES[name], name


def kernels(text):
    """(name, body) of every __global__ function of a source"""
    return [(m.group(1), text[m.end():].split('\n}\n')[0]) for m in re.finditer(r'__global__[^\n;{]*\bvoid (\w+)\(', text)]


def reach_text(name):
    """a source with the csrc headers it reaches"""
    return SOURCES[name] + ''.join(SOURCES[n] for n in reach(name))


def reach(name, seen=None):
    """the csrc headers `name` includes, directly or through others"""
    seen = set() if seen is None else seen
    for inc in re.findall(r'#include "([^"/]+)"', SOURCES[name]):
        if inc not in seen:
            seen.add(inc)
            reach(inc, seen)
    return seen


def test_no_check_header_reaches_the_device_header_and_the_common_one_is_plain_cpp():
    for name in SOURCES:
        if name.endswith('_check.h'):
            assert DEVICE not in reach(name), name
    chk = SOURCES[CHECK]
    assert not re.search(r'#include\s*[<"][^>"]*hip', chk) and 'hip_runtime' not in chk and not re.findall(r'#include "', chk)
    assert '#include <hip/hip_runtime.h>' in SOURCES[DEVICE]
