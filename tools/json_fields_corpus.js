'use strict'
// Keyed-object corpus for ygm_json_fields_v1 (test tooling): what TiptapTransformer.fromYdoc(doc, fields) gives for a
// stored document when `fields` is undefined / [] (every key of doc.share) or a list of names:
//     data = {}; fields.forEach(field => { data[field] = yDocToProsemirrorJSON(doc, field) }); JSON.stringify(data)
// with y-prosemirror's serializer restated over yjs 13.5.16 as in tools/json_corpus.js, whose `serialize`, `jsonOf`
// and refusal rules are required from there (that tool's output does not change).
// For every state of the five snapshot fixtures the asks recorded are: all fields, and a listed ask -- the share keys
// reversed, then one absent name, then the first listed name once more.  Most of those states hold roots of other
// kinds (texts, maps, arrays with content), which refuse as fragments, so a third ask lists, reversed, the roots that
// do serialize (when the state has any): the objects of several keys come from there.  The edge sessions are
// generated here and carry their own states and asks.  A row is
//     [fields, status, jsonHex]            fields: null (all) or [nameHex, ...] in list order
//     [fields, status, sha256, length]     past the first FULL states of a set
// Each state also records `keys`: the share keys (hex) in JavaScript's own-property order, the key order of its
// all-fields object.  The states are not stored again (row i belongs to row i of the input fixture).
// Statuses (include/ygm.h): the state's own refusal first; then the first refusing field in output order -- index
// keys ascending, then the others by first assignment -- a field named __proto__ being YGM_EUNSUPPORTED (9) where it
// stands in that order.
//   node tools/json_fields_corpus.js <out.json.gz> [limit]
const fs = require('fs')
const path = require('path')
const zlib = require('zlib')
const crypto = require('crypto')
const Y = require(path.join(__dirname, 'yjs_bundle.js')).load()
const { jsonOf, Refuse } = require(path.join(__dirname, 'json_corpus.js'))

const GOLDEN = path.join(__dirname, '..', 'tests', 'golden')
const SETS = ['snapshot_v135', 'snapshot_text_v135', 'snapshot_pending_v135', 'snapshot_subdoc_v135', 'snapshot_nogc_v135']
const ABSENT = 'no-such-root'
const FULL = 40
const hex = s => Buffer.from(s, 'utf8').toString('hex')

// the state's refusal whatever is asked (json_corpus.js's stateRefusal is not exported: the same rule, see there)
const sigDigits = v => String(Math.abs(v)).replace(/^0\./, '').replace(/\./, '').replace(/^0+/, '').replace(/0+$/, '').length
function stateRefusal (doc) {
  let st = 0
  const json = v => {
    if (typeof v === 'number') { if (Number.isFinite(v) && (/e/.test(String(v)) || sigDigits(v) > 15)) st = 3 } else if (Array.isArray(v)) v.forEach(json)
    else if (v !== null && typeof v === 'object') Object.keys(v).forEach(k => json(v[k]))
  }
  const any = v => {
    if (typeof v === 'number') { if (Number.isInteger(v) && v < -2147483647) st = 3 } else if (Array.isArray(v)) v.forEach(any)
    else if (v !== null && typeof v === 'object' && !(v instanceof Uint8Array)) Object.keys(v).forEach(k => any(v[k]))
  }
  doc.store.clients.forEach(structs => structs.forEach(it => {
    if (it.content === undefined) return
    const ref = it.content.getRef()
    if (ref === 6) json(it.content.value)
    else if (ref === 5) json(it.content.embed)
    else if (ref === 8) it.content.arr.forEach(any)
  }))
  return st
}

// own-property order of data[name] = ... assignments made in list order.  (An object without a prototype: there
// "__proto__" is a key like any other, so its place in the order can be read; the order rule is the engine's V8's.)
function keyOrder (names) {
  const o = Object.create(null)
  names.forEach(n => { o[n] = true })
  return Object.keys(o)
}
const shareKeys = state => { const d = new Y.Doc(); Y.applyUpdate(d, state); return Array.from(d.share.keys()) }

// [status, json] of fromYdoc(doc, fields) for fields = null (all) or an array of names
function fieldsOf (state, fields) {
  const doc = new Y.Doc()
  Y.applyUpdate(doc, state)
  const whole = stateRefusal(doc)
  if (whole) return [whole, '']
  const list = fields === null || fields.length === 0 ? Array.from(doc.share.keys()) : fields
  const parts = new Map()
  for (const name of keyOrder(list)) {   // the first refusal in output order
    if (name === '__proto__') return [9, '']
    try { parts.set(name, jsonOf(doc, name)) } catch (e) { if (!(e instanceof Refuse)) throw e; return [e.st, ''] }
  }
  const data = {}   // the reference's own loop: the assignments in list order on a plain object
  list.forEach(field => { data[field] = JSON.parse(parts.get(field)) })
  const text = JSON.stringify(data)
  // the same object put together from the single-field JSONs, in the recorded key order
  const joined = '{' + keyOrder(list).map(k => JSON.stringify(k) + ':' + parts.get(k)).join(',') + '}'
  if (joined !== text) throw new Error('the key order rule does not hold for ' + JSON.stringify(list))
  return [0, text]
}
// the share keys that serialize as fragments, reversed ([]: none, or the state itself is refused)
function goodAsk (state, keys) {
  const doc = new Y.Doc()
  Y.applyUpdate(doc, state)
  if (stateRefusal(doc)) return []
  return keys.filter(k => { if (k === '__proto__') return false; try { jsonOf(doc, k); return true } catch (e) { if (!(e instanceof Refuse)) throw e; return false } }).reverse()
}
const listedAsk = keys => { const l = keys.slice().reverse(); l.push(ABSENT); l.push(l[0]); return l }
const row = (fields, r, full) => {
  const f = fields === null ? null : fields.map(hex)
  if (full) return [f, r[0], Buffer.from(r[1], 'utf8').toString('hex')]
  const b = Buffer.from(r[1], 'utf8')
  return [f, r[0], crypto.createHash('sha256').update(b).digest('hex'), b.length]
}

// ---- edge sessions: { note, state, asks: [fields ...] }
const el = (parent, at, nodeName) => { const e = new Y.XmlElement(nodeName); parent.insert(at, [e]); return e }
const txt = (parent, at, s, attrs) => { const t = new Y.XmlText(); parent.insert(at, [t]); if (s !== null) t.insert(0, s, attrs); return t }
const para = (parent, at, s) => { const e = el(parent, at, 'paragraph'); if (s !== null) txt(e, 0, s); return e }
const ODD = ['2', '10', 'b', '01', '', '4294967295', 'a"\\\n\u0001é']

function edges () {
  const out = []
  const one = (note, id, f, asks) => { const d = new Y.Doc(); d.clientID = id; f(d); out.push({ note, state: Y.encodeStateAsUpdate(d), asks }) }
  one('no roots', 301, d => {}, [null, ['a'], ['a', 'a'], ['']])
  one('one root', 302, d => { para(d.getXmlFragment('default'), 0, 'only') }, [null, ['default'], ['default', 'default'], [ABSENT, 'default']])
  one('roots named 2, 10, b, 01, the empty name, 4294967295 and a name to escape', 303, d => {
    ODD.forEach((n, i) => para(d.getXmlFragment(n), 0, 'in ' + i))
  }, [null, listedAsk(ODD), ['b', '10', '2', '10', 'b', '9', ''], ['4294967295', '4294967294', '0', '00']])
  one('a __proto__ root', 304, d => { para(d.getXmlFragment('first'), 0, 'x'); para(d.getXmlFragment('__proto__'), 0, 'y'); para(d.getXmlFragment('7'), 0, 'z') },
    [null, ['first', '__proto__'], ['__proto__'], ['first', '7'], ['__proto_', '__proto__x', 'first']])
  one('two roots, the second refuses with 9', 305, d => { para(d.getXmlFragment('good'), 0, 'x'); d.getXmlFragment('bad').insert(0, [new Y.Map()]) },
    [null, ['good', 'bad'], ['bad', 'good'], ['good'], ['good', '__proto__', 'bad'], ['bad', '__proto__']])
  one('two roots, the first in output order refuses with 3, the other with 9', 306, d => {
    d.getXmlFragment('z').insert(0, [new Y.Map()])
    para(d.getXmlFragment('1'), 0, 'x').setAttribute('w', 1.5)
  }, [null, ['z', '1'], ['1', 'z'], ['z'], ['__proto__', '1'], ['1', '__proto__']])
  one('a map-only root beside a fragment', 307, d => { d.getMap('meta').set('k', 1); para(d.getXmlFragment('default'), 0, 'x') }, [null, ['meta'], ['default', 'meta']])
  one('a Y.Text root beside a fragment root', 308, d => { d.getText('title').insert(0, 'plain'); para(d.getXmlFragment('default'), 0, 'x') },
    [null, ['default'], ['title'], ['default', 'title']])
  one('an empty Y.Text root beside a fragment root', 309, d => { const t = d.getText('title'); t.insert(0, 'gone'); t.delete(0, 4); para(d.getXmlFragment('default'), 0, 'x') },
    [null, ['title', 'default']])
  {   // a root that only pending structs name: the update that would have joined the later ones to the state is lost
    const a = new Y.Doc(); a.clientID = 310
    const log = []
    a.on('update', u => log.push(u))
    a.transact(() => para(a.getXmlFragment('base'), 0, 'kept'))
    a.transact(() => para(a.getXmlFragment('base'), 1, 'lost'))
    a.transact(() => para(a.getXmlFragment('late'), 0, 'pending'))
    if (log.length !== 3) throw new Error('one update per transaction expected')
    const kept = [log[0], log[2]]   // (the 'lost' paragraph's update is gone: 'late' waits for it)
    out.push({ note: 'a root named only by pending structs', state: Y.mergeUpdates(kept), asks: [null, ['late'], ['late', 'base']] })
  }
  {   // the roots fit their workspace's output region one by one, the object does not: growing marks, as the single-field
      // overflow session, shared out over several roots
    const d = new Y.Doc(); d.clientID = 311
    for (let r = 0; r < 6; r++) {
      const t = txt(para(d.getXmlFragment('root-' + r), 0, null), 0, null)
      const attrs = {}
      for (let i = 0; i < 40; i++) { attrs['mark-number-' + i] = { n: i, s: 'value-' + i }; t.insert(i, String.fromCharCode(65 + (i % 26)), Object.assign({}, attrs)) }
    }
    out.push({ note: 'overflow: six roots that fit one by one, an object that does not', state: Y.encodeStateAsUpdate(d), asks: [null, ['root-5', 'root-0']] })
  }
  return out
}

// snap::caps_of(S, D, C, n).out = n + 48 (3 S + 2 D + 4) + 16 (C + 1) + 64
function capsOut (state) {
  const d = new Y.Doc(); Y.applyUpdate(d, state)
  let S = 0; let D = 0
  d.store.clients.forEach(structs => { S += structs.length })
  Y.createDeleteSetFromStructStore(d.store).clients.forEach(ranges => { D += ranges.length })
  return state.length + 48 * (3 * S + 2 * D + 4) + 16 * (d.store.clients.size + 1) + 64
}

if (require.main === module) {
  const limit = process.argv[3] ? parseInt(process.argv[3], 10) : Infinity
  const inputs = {}
  const sets = {}
  const counts = {}
  for (const s of SETS) {
    const raw = fs.readFileSync(path.join(GOLDEN, s + '.json.gz'))
    inputs[s + '.json.gz'] = crypto.createHash('sha256').update(raw).digest('hex')
    const rows = JSON.parse(zlib.gunzipSync(raw).toString()).rows
    const c = { states: 0, ok_all: 0, ok_listed: 0, good: 0, good_multi: 0, multi: 0, index_keys: 0 }
    sets[s] = rows.slice(0, limit).map((r, i) => {
      const state = Buffer.from(r[0], 'hex')
      const keys = shareKeys(state)
      const listed = listedAsk(keys)
      const all = fieldsOf(state, null)
      const some = fieldsOf(state, listed)
      c.states++
      if (all[0] === 0) c.ok_all++
      if (some[0] === 0) c.ok_listed++
      if (keys.length >= 2) c.multi++
      if (keyOrder(keys).join('\u0000') !== keys.join('\u0000')) c.index_keys++
      const asks = [row(null, all, i < FULL), row(listed, some, i < FULL)]
      const good = goodAsk(state, keys)
      if (good.length) {
        const g = fieldsOf(state, good)
        if (g[0] !== 0) throw new Error('a list of serializable roots was refused')
        asks.push(row(good, g, i < FULL))
        c.good++
        if (good.length >= 2) c.good_multi++
      }
      return { keys: keyOrder(keys).map(hex), asks }
    })
    counts[s] = c
  }
  const edge = edges().map(e => ({
    note: e.note,
    state: Buffer.from(e.state).toString('hex'),
    keys: keyOrder(shareKeys(e.state)).map(hex),
    asks: e.asks.map(f => row(f, fieldsOf(e.state, f), true))
  }))
  const doc = {
    source: 'tools/json_fields_corpus.js (yjs 13.5.16 bundle; y-prosemirror restated): node tools/json_fields_corpus.js tests/golden/json_fields_v135.json.gz',
    absent: hex(ABSENT),
    full: FULL,
    inputs,
    counts,
    sets,
    edges: edge
  }
  fs.writeFileSync(process.argv[2], zlib.gzipSync(Buffer.from(JSON.stringify(doc)), { level: 9 }))
  const ovf = edges().filter(e => e.note.startsWith('overflow'))[0]
  const od = new Y.Doc(); Y.applyUpdate(od, ovf.state)
  const per = Array.from(od.share.keys()).map(k => Buffer.byteLength(jsonOf(od, k), 'utf8'))
  console.log(JSON.stringify({ counts, edges: edge.length, overflow_caps_out: capsOut(ovf.state), overflow_root_bytes: per, overflow_object_bytes: Buffer.byteLength(fieldsOf(ovf.state, null)[1], 'utf8') }))
}

module.exports = { fieldsOf, keyOrder, listedAsk }
