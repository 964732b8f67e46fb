'use strict'
// toJSON corpus for ygm_tojson_v1 (test tooling): what a stored document's Map, Array or Text root is, as yjs 13.5.16
// (the image's bundle, tools/yjs_bundle.js) serializes it:
//   JSON.stringify(doc.getMap(name).toJSON()) / doc.getArray(name).toJSON() / doc.getText(name).toJSON()
// for doc = Y.applyUpdate(new Y.Doc(), state), or a refusal of include/ygm.h's table (9 YGM_EUNSUPPORTED,
// 3 YGM_ENONCANON, 1 YGM_EMALFORMED for a BigInt) with no bytes.  The JSON is the bundle's own toJSON; `check` below
// only decides whether the engine refuses the root, by walking the types as the table reads.
// The fixture holds
//   edges    sessions named for what they show: { note, state, asks: [[nameHex, kind, status, jsonHex], ...] }
//   random   seeded sessions (the PRNG is mulberry32 below): 2-3 clients doing Map / Array / Text operations with
//            concurrent sets and deletes, their updates applied in a random order; roots m / a / t asked as their kind
//   sets     the roots of five committed snapshot fixtures (the `u` of each row; the states are not stored again: row i
//            belongs to row i of the input fixture, whose sha256 is recorded) and one absent name, each asked as all
//            three kinds: [nameHex, kind, status, jsonHex], past the first FULL states [nameHex, kind, status, sha256,
//            length]
//   node tools/tojson_corpus.js <out.json.gz> [limit]     (limit: only the first `limit` states of each set)
//   node tools/tojson_corpus.js --time <fixture.json.gz> <count>
//        the CPU path this replaces, on one core: JSON.stringify(applyUpdate(new Doc, s).getMap(n).toJSON()) over the
//        random sessions' map asks repeated to <count> documents.  One JSON line.
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const crypto = require('crypto')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()

const GOLDEN = path.join(__dirname, '..', 'tests', 'golden')
const SETS = ['snapshot_v135', 'snapshot_text_v135', 'snapshot_pending_v135', 'snapshot_subdoc_v135', 'snapshot_nogc_v135']
const ABSENT = 'no-such-root'
const FULL = 40
const MAP = 0; const ARRAY = 1; const TEXT = 2
const SESSIONS = 160
const ESCAPES = 'q" b\\ \b\f\n\r\t \u0001\u001f \u007f \u2028 😀'   // (the string of json_v135's "values of every kind")

class Refuse extends Error { constructor (st) { super('refused ' + st); this.st = st } }
// the refusal table of a context opened with YGM_F_FLOATS (tools/floats_corpus.js turns it on; this tool's own fixture
// is made with it off)
let FLOATS = false
const setFloats = on => { FLOATS = !!on }

// ---- does the engine refuse the root?  (include/ygm.h's table, in the order of the engine's walk)
function checkAny (v) {
  if (typeof v === 'bigint') throw new Refuse(1)
  if (typeof v === 'number') { if (!FLOATS && Number.isFinite(v) && (!Number.isInteger(v) || Math.abs(v) > 9007199254740992)) throw new Refuse(3) } else if (v instanceof Uint8Array) throw new Refuse(9)
  else if (Array.isArray(v)) v.forEach(checkAny)
  else if (v !== null && typeof v === 'object') Object.keys(v).forEach(k => checkAny(v[k]))
}
function checkNested (t) {
  if (t.constructor === Y.Array) checkType(t, ARRAY)
  else if (t.constructor === Y.Map) checkType(t, MAP)
  else if (t.constructor !== Y.Text) throw new Refuse(9)
}
// Map: index keys ascending, then _map order (the order the engine writes, and so refuses, in)
function mapOrder (type) {
  const keys = []
  type._map.forEach((item, key) => { if (!item.deleted) keys.push(key) })
  const isIndex = k => /^(0|[1-9][0-9]{0,9})$/.test(k) && Number(k) < 4294967295
  return keys.filter(isIndex).sort((a, b) => Number(a) - Number(b)).concat(keys.filter(k => !isIndex(k)))
}
function checkType (type, kind) {
  if (kind === TEXT) return
  if (kind === MAP) {
    for (const key of mapOrder(type)) {
      const item = type._map.get(key)
      const ref = item.content.getRef()
      if (ref !== 8 && ref !== 2 && ref !== 7) throw new Refuse(9)
      if (key === '__proto__') throw new Refuse(9)
      if (ref === 7) checkNested(item.content.type)
      else checkAny(item.content.getContent()[item.length - 1])
    }
    return
  }
  for (let item = type._start; item !== null; item = item.right) {
    if (item.deleted || !item.countable) continue
    const ref = item.content.getRef()
    if (ref === 7) checkNested(item.content.type)
    else if (ref === 8 || ref === 2) item.content.getContent().forEach(checkAny)
    else throw new Refuse(9)
  }
}
const rootOf = (doc, name, kind) => kind === MAP ? doc.getMap(name) : kind === ARRAY ? doc.getArray(name) : doc.getText(name)

// [nameHex, kind, status, json (utf8 string)] of one ask (a fresh document per ask: get* fixes a root's type)
function ask (state, name, kind) {
  const doc = new Y.Doc()
  Y.applyUpdate(doc, state)
  const root = rootOf(doc, name, kind)
  const hex = Buffer.from(name, 'utf8').toString('hex')
  try {
    checkType(root, kind)
    return [hex, kind, 0, JSON.stringify(root.toJSON())]
  } catch (e) {
    if (!(e instanceof Refuse)) throw e
    return [hex, kind, e.st, '']
  }
}
const fullRow = r => [r[0], r[1], r[2], Buffer.from(r[3], 'utf8').toString('hex')]
const hashRow = r => { const b = Buffer.from(r[3], 'utf8'); return [r[0], r[1], r[2], crypto.createHash('sha256').update(b).digest('hex'), b.length] }

// ---- edge sessions
function edges () {
  const out = []
  const push = (note, state, asks) => {
    try {
      out.push({ note, state: Buffer.from(state).toString('hex'), asks: asks.map(([n, k]) => fullRow(ask(state, n, k))) })
    } catch (e) { e.message = note + ': ' + e.message; throw e }
  }
  const one = (note, id, f, asks) => { const d = new Y.Doc(); d.clientID = id; f(d); push(note, Y.encodeStateAsUpdate(d), asks) }
  const ALL = n => [[n, MAP], [n, ARRAY], [n, TEXT]]
  const two = (ida, idb, first) => {
    const a = new Y.Doc(); a.clientID = ida
    const b = new Y.Doc(); b.clientID = idb
    first(a)
    Y.applyUpdate(b, Y.encodeStateAsUpdate(a))
    return [a, b]
  }
  one('an empty root, as each kind', 301, d => { d.getMap('m').set('k', 1); d.getMap('m').delete('k'); d.getArray('a').push([1]); d.getArray('a').delete(0, 1); d.getText('t').insert(0, 'x'); d.getText('t').delete(0, 1) }, [['m', MAP], ['a', ARRAY], ['t', TEXT]])
  one('an absent root, as each kind', 302, d => { d.getMap('m').set('k', 1) }, ALL(ABSENT))
  one('keys "10", "9", "a", "04" set in that order', 303, d => { for (const k of ['10', '9', 'a', '04']) d.getMap('m').set(k, 'v' + k) }, [['m', MAP]])
  one('a key set twice', 304, d => { const m = d.getMap('m'); m.set('a', 'one'); m.set('b', 'two'); m.set('a', 'three') }, [['m', MAP]])
  one('a key set then deleted, alone', 305, d => { const m = d.getMap('m'); m.set('a', 'one'); m.delete('a') }, [['m', MAP]])
  one('a key set then deleted beside a live one', 306, d => { const m = d.getMap('m'); m.set('a', 'one'); m.set('b', 'two'); m.delete('a') }, [['m', MAP]])
  {
    const [a, b] = two(307, 308, a => a.getMap('m').set('first', 'f'))
    a.getMap('m').set('k', 'from-a'); b.getMap('m').set('k', 'from-b'); b.getMap('m').set('only-b', 1)
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    push('two clients setting one key concurrently', Y.encodeStateAsUpdate(a), [['m', MAP]])
  }
  one('a value undefined in a Map', 309, d => { const m = d.getMap('m'); m.set('a', 1); m.set('u', undefined); m.set('b', 2) }, [['m', MAP]])
  one('undefined inside an Any object and an Any array', 310, d => { d.getMap('m').set('o', { z: undefined, y: [undefined, 1] }); d.getArray('a').push([[undefined], { only: undefined }]) }, [['m', MAP], ['a', ARRAY]])
  {   // hand-made (13.5.16's Y.Array refuses to insert undefined and never writes a ContentJSON, but reads both): client 350,
      // root 'a': ContentAny [undefined, 1] then ContentJSON ['{"a":1}', 'undefined', '7']; root 'm': key 'k' ContentJSON ['"v"'],
      // key 'u' ContentJSON ['undefined']
    const str = s => [s.length].concat(Array.from(Buffer.from(s, 'latin1')))
    const u = [1, 4, 0xDE, 0x02, 0].concat([8, 1], str('a'), [2, 127, 125, 1])
      .concat([0x82, 0xDE, 0x02, 1, 3], str('{"a":1}'), str('undefined'), str('7'))
      .concat([0x22, 1], str('m'), str('k'), [1], str('"v"'))
      .concat([0x22, 1], str('m'), str('u'), [1], str('undefined'))
      .concat([0])
    push('an undefined Array element and ContentJSON elements', Uint8Array.from(u), [['a', ARRAY], ['m', MAP]])
  }
  one('values of every kind', 311, d => {
    const m = d.getMap('m')
    m.set('s', ESCAPES); m.set('n', -42); m.set('nz', -0); m.set('t', true); m.set('f', false); m.set('z', null)
    m.set('o', { k: [1, 'two', { deep: null }], '2': 'index', e: {} }); m.set('arr', [[], {}, 0])
    d.getArray('a').push([ESCAPES, -42, -0, true, false, null, { k: [1, 'two', { deep: null }], '2': 'index', e: {} }, [[], {}, 0]])
  }, [['m', MAP], ['a', ARRAY]])
  one('numbers 1700000000000, 4294967296, 2^53, Infinity, NaN', 312, d => {
    const m = d.getMap('m')
    m.set('now', 1700000000000); m.set('u32', 4294967296); m.set('big', 9007199254740992);
    m.set('inf', Infinity); m.set('ninf', -Infinity); m.set('nan', NaN); m.set('in', { at: [1700000000001, NaN] })
    d.getArray('a').push([1700000000000, 4294967296, 9007199254740992, Infinity, NaN])
  }, [['m', MAP], ['a', ARRAY]])
  one('Array items of several elements with a deleted run in the middle', 313, d => { const a = d.getArray('a'); a.push([1, 2, 3, 4, 5]); a.push(['six', { seven: 7 }, [8]]); a.insert(0, [0]); a.delete(3, 4) }, [['a', ARRAY]])
  one('Map in Array in Map, 40 deep', 314, d => {
    let p = d.getMap('m')
    for (let i = 0; i < 40; i++) {
      if (i % 2 === 0) { const a = new Y.Array(); p.set('k' + i, a); if (i % 6 === 0) p.set('beside' + i, i); p = a } else { const m = new Y.Map(); p.push(['before' + i, m]); p = m }
    }
    p.set('bottom', 'here')
  }, [['m', MAP]])
  one('a nested Text with formats, an embed and a deleted middle', 315, d => {
    const t = new Y.Text()
    d.getMap('m').set('t', t)
    t.insert(0, 'plain bold MIDDLE tail'); t.format(6, 4, { bold: true }); t.insertEmbed(5, { image: 'x.png' }); t.delete(12, 7)
    const t2 = new Y.Text('in "array"\n')
    d.getArray('a').push([t2, 'next'])
  }, [['m', MAP], ['a', ARRAY]])
  {
    const [a, b] = two(316, 317, a => a.getText('t').insert(0, 'a😀b'))
    b.getText('t').insert(2, 'X'); a.getText('t').insert(4, 'tail')
    Y.applyUpdate(a, Y.encodeStateAsUpdate(b))
    push('a Text cut through a surrogate pair', Y.encodeStateAsUpdate(a), [['t', TEXT]])
  }
  one('a Text root with every escape class', 318, d => { d.getText('t').insert(0, ESCAPES + ' end') }, [['t', TEXT]])
  one('a root holding both map entries and list items, asked as each kind', 319, d => {
    const t = d.getText('r')
    t.insert(0, 'text'); t.setAttribute('attr', { v: 1 })
  }, ALL('r'))
  {   // two peers, then a lost update (pending structs with an integrated part)
    const [a, b] = two(320, 321, a => { a.getMap('m').set('shared', 'start'); a.getArray('a').push(['one']) })
    const log = []
    a.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    b.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    const base = Y.encodeStateAsUpdate(a)
    a.getMap('m').set('from-a', 1); b.getMap('m').set('from-b', { n: 2 })
    a.getArray('a').push(['two']); a.getArray('a').push(['lost']); a.getArray('a').push(['after-the-gap'])
    const lost = log.slice(); lost.splice(lost.length - 2, 1)
    push('a state with pending structs', Y.mergeUpdates([base].concat(lost)), [['m', MAP], ['a', ARRAY]])
  }
  one('a 4 KB string of 0x01 bytes in a Map', 322, d => { d.getMap('m').set('ctl', '\u0001'.repeat(4096)) }, [['m', MAP]])
  // refusals: one per row of the header's table
  one('refused: a nested XmlElement', 331, d => { d.getMap('m').set('ok', 1); d.getMap('m').set('x', new Y.XmlElement('p')) }, [['m', MAP]])
  one('refused: a nested XmlFragment, XmlHook and XmlText in an Array', 332, d => { d.getArray('a').push([new Y.XmlFragment()]); d.getArray('b').push([new Y.XmlHook('h')]); d.getArray('c').push([new Y.XmlText('x')]) }, [['a', ARRAY], ['b', ARRAY], ['c', ARRAY]])
  one('refused: a ContentBinary in an Array', 333, d => { d.getArray('a').push([1, new Uint8Array([1, 2, 3])]) }, [['a', ARRAY]])
  one('refused: a Uint8Array inside an Any', 334, d => { d.getMap('m').set('o', { bin: new Uint8Array([1, 2, 3]) }) }, [['m', MAP]])
  one('refused: a ContentDoc', 335, d => { d.getMap('m').set('sub', new Y.Doc({ guid: 'sub-doc-guid' })) }, [['m', MAP]])
  one('refused: a live ContentString in an Array\'s list', 336, d => { d.getText('t').insert(0, 'abc') }, [['t', ARRAY]])
  one('refused: a live ContentEmbed in an Array\'s list', 337, d => { d.getText('t').insertEmbed(0, { rule: true }) }, [['t', ARRAY]])
  one('refused: a live Map entry that is a ContentBinary', 338, d => { d.getMap('m').set('bin', new Uint8Array([9])) }, [['m', MAP]])
  one('refused: a Y.Map key __proto__ with a live entry', 339, d => { d.getMap('m').set('a', 1); d.getMap('m').set('__proto__', { x: 1 }) }, [['m', MAP]])
  one('refused: a finite non-integer number', 340, d => { d.getMap('m').set('w', 1.5); d.getArray('a').push([{ deep: [0.25] }]) }, [['m', MAP], ['a', ARRAY]])
  one('refused: an integer above 2^53', 341, d => { d.getMap('m').set('w', 1152921504606846976) }, [['m', MAP]])
  if (typeof BigInt === 'function') one('refused: a BigInt', 342, d => { d.getMap('m').set('big', { n: BigInt(5) }) }, [['m', MAP]])
  return out
}

// ---- seeded random sessions
function mulberry32 (a) {
  return () => {
    a |= 0; a = a + 0x6D2B79F5 | 0
    let t = Math.imul(a ^ a >>> 15, 1 | a)
    t = t + Math.imul(t ^ t >>> 7, 61 | t) ^ t
    return ((t ^ t >>> 14) >>> 0) / 4294967296
  }
}
const KEYS = ['title', 'id', 'x', 'y', 'color', 'done', 'tags', 'meta', '0', '7', '12', 'updatedAt', 'owner', 'k"q']
const WORDS = ['alpha', 'beta', 'gamma "quoted"', 'delta\n', 'épsilon', 'zeta😀', 'eta\\', 'theta', 'a longer piece of text for a card body', '']
function randomSession (seed, forceFloaty) {   // forceFloaty: every session holds non-integer numbers (tools/floats_corpus.js)
  const rnd = mulberry32(seed)
  const int = n => Math.floor(rnd() * n)
  const pick = a => a[int(a.length)]
  const floaty = rnd() < 0.05 || !!forceFloaty   // (a session with a non-integer number: its roots are refused where it is reached)
  const scalar = () => {
    const r = int(10)
    if (r < 3) return pick(WORDS)
    if (r < 5) return int(2000) - 1000
    if (r === 5) return 1700000000000 + int(100000000)
    if (r === 6) return rnd() < 0.5
    if (r === 7) return null
    if (r === 8) return floaty ? int(100) + 0.5 : int(100)
    return rnd() < 0.2 ? undefined : pick(WORDS) + int(100)
  }
  const value = depth => {
    const r = int(8)
    if (depth > 2 || r < 5) return scalar()
    if (r < 7) { const o = {}; for (let i = int(4); i >= 0; i--) o[pick(KEYS)] = value(depth + 1); return o }
    const a = []; for (let i = int(4); i >= 0; i--) a.push(value(depth + 1)); return a
  }
  const elem = () => { const v = value(0); return v === undefined ? null : v }   // (Y.Array refuses to insert undefined)
  const nested = () => {
    const r = int(3)
    if (r === 0) { const m = new Y.Map(); return [m, () => { for (let i = int(3); i >= 0; i--) m.set(pick(KEYS), value(0)) }] }
    if (r === 1) { const a = new Y.Array(); return [a, () => { a.push([elem(), elem()]) }] }
    const t = new Y.Text(); return [t, () => { t.insert(0, pick(WORDS) + ' ' + pick(WORDS)) }]
  }
  const n = 2 + int(2)
  const docs = []; const log = []
  for (let i = 0; i < n; i++) {
    const d = new Y.Doc(); d.clientID = 1000 + 10 * (seed % 100000) + i
    d.on('update', (u, o, doc, tr) => { if (tr.local) log.push(u) })
    docs.push(d)
  }
  const mapOp = m => {
    const r = int(10)
    if (r < 6) m.set(pick(KEYS), value(0))
    else if (r < 8) { const ks = Array.from(m.keys()); if (ks.length) m.delete(pick(ks)) } else { const [t, fill] = nested(); m.set(pick(KEYS), t); fill() }
  }
  const arrayOp = a => {
    const r = int(10)
    if (r < 5) { const vs = []; for (let i = int(3); i >= 0; i--) vs.push(elem()); a.insert(int(a.length + 1), vs) } else if (r < 8) { if (a.length) { const at = int(a.length); a.delete(at, 1 + int(Math.min(3, a.length - at))) } } else { const [t, fill] = nested(); a.insert(int(a.length + 1), [t]); fill() }
  }
  const textOp = t => {
    const r = int(10)
    if (r < 6) t.insert(int(t.length + 1), pick(WORDS))
    else if (r < 8) { if (t.length) { const at = int(t.length); t.delete(at, 1 + int(Math.min(4, t.length - at))) } } else if (t.length) t.format(0, 1 + int(t.length), { bold: rnd() < 0.5 ? true : null })
  }
  const into = (d, f) => {   // one operation on a root or, sometimes, on a nested type of it
    const r = int(3)
    if (r === 0) {
      let m = d.getMap('m')
      const inner = Array.from(m.values()).filter(v => v instanceof Y.Map)
      if (inner.length && rnd() < 0.3) m = pick(inner)
      mapOp(m)
    } else if (r === 1) {
      let a = d.getArray('a')
      const inner = a.toArray().filter(v => v instanceof Y.Array)
      if (inner.length && rnd() < 0.3) a = pick(inner)
      arrayOp(a)
    } else textOp(d.getText('t'))
  }
  const rounds = 3 + int(4)
  for (let r = 0; r < rounds; r++) {
    for (const d of docs) for (let i = int(4); i >= 0; i--) into(d)
    if (rnd() < 0.6) {   // some peers hear of each other between rounds; the rest stays concurrent
      const a = pick(docs); const b = pick(docs)
      if (a !== b) { Y.applyUpdate(b, Y.encodeStateAsUpdate(a)); Y.applyUpdate(a, Y.encodeStateAsUpdate(b)) }
    }
  }
  for (let i = log.length - 1; i > 0; i--) { const j = int(i + 1); const t = log[i]; log[i] = log[j]; log[j] = t }
  const merged = new Y.Doc()
  for (const u of log) Y.applyUpdate(merged, u)
  const state = Y.encodeStateAsUpdate(merged)
  return { seed, state: Buffer.from(state).toString('hex'), asks: [['m', MAP], ['a', ARRAY], ['t', TEXT]].map(([nm, k]) => fullRow(ask(state, nm, k))) }
}

function timeAsks (file, count) {
  const fix = JSON.parse(zlib.gunzipSync(fs.readFileSync(file)).toString())
  const asks = []
  for (const s of fix.random) for (const r of s.asks) if (r[1] === MAP && r[2] === 0) asks.push([Buffer.from(s.state, 'hex'), Buffer.from(r[0], 'hex').toString('utf8')])
  let best = Infinity; let bytes = 0
  for (let rep = 0; rep < 3; rep++) {
    bytes = 0
    const t0 = process.hrtime.bigint()
    for (let i = 0; i < count; i++) {
      const [state, name] = asks[i % asks.length]
      const doc = new Y.Doc()
      Y.applyUpdate(doc, state)
      bytes += Buffer.byteLength(JSON.stringify(doc.getMap(name).toJSON()), 'utf8')
    }
    best = Math.min(best, Number(process.hrtime.bigint() - t0) / 1e6)
  }
  console.log(JSON.stringify({ docs: count, distinct: asks.length, json_bytes: bytes, yjs_ms: Math.round(best * 100) / 100 }))
}

if (require.main === module && process.argv[2] === '--time') {
  timeAsks(process.argv[3], parseInt(process.argv[4], 10))
} else if (require.main === module) {
  const limit = process.argv[3] ? parseInt(process.argv[3], 10) : Infinity
  const inputs = {}
  const sets = {}
  const counts = {}
  for (const s of SETS) {
    const raw = fs.readFileSync(path.join(GOLDEN, s + '.json.gz'))
    inputs[s + '.json.gz'] = crypto.createHash('sha256').update(raw).digest('hex')
    const rows = JSON.parse(zlib.gunzipSync(raw).toString()).rows
    const c = { states: 0, asks: 0, ok: 0, refused: 0, trivial: 0 }
    sets[s] = rows.slice(0, limit).map((r, i) => {
      const state = Buffer.from(r[0], 'hex')
      const probe = new Y.Doc()
      Y.applyUpdate(probe, state)
      const names = Array.from(probe.share.keys())
      names.push(ABSENT)
      c.states++
      const x = []
      for (const name of names) {
        for (const kind of [MAP, ARRAY, TEXT]) {
          const q = ask(state, name, kind)
          c.asks++
          if (q[2] === 0) { c.ok++; if (q[3] === '{}' || q[3] === '[]' || q[3] === '""') c.trivial++ } else c.refused++
          x.push(q)
        }
      }
      return x.map(i < FULL ? fullRow : hashRow)
    })
    counts[s] = c
  }
  const random = []
  for (let i = 0; i < SESSIONS; i++) random.push(randomSession(20240 + 7 * i))
  const rr = [].concat(...random.map(s => s.asks))
  const ok = rr.filter(r => r[2] === 0)
  counts.random = { sessions: random.length, asks: rr.length, ok: ok.length, over64: ok.filter(r => r[3].length / 2 > 64).length }
  const edge = edges()
  const doc = {
    source: 'tools/tojson_corpus.js (yjs 13.5.16 bundle): node tools/tojson_corpus.js tests/golden/tojson_v135.json.gz',
    absent: Buffer.from(ABSENT, 'utf8').toString('hex'),
    full: FULL,
    inputs,
    counts,
    sets,
    random,
    edges: edge
  }
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  console.log(JSON.stringify({ counts, edges: edge.length }))
}

module.exports = { ask, Refuse, edges, randomSession, setFloats, MAP, ARRAY, TEXT }
